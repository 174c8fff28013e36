"""The restarted block GCR of Engine::bgcr_tile (block GMRES(m) with right preconditioning in exact arithmetic, the residual
kept factored and rank-revealed as block CG keeps it) restated in numpy around a solve(r) callback, in the order of
operations of the device, and the inputs the GPU tests use (test_blockgcr_host.py pins them on the CPU,
test_gpu_blockgcr.py holds the driver against them).  numpy / scipy only.

trace (a list) receives one dict per tile: `cycles` = one dict per cycle start with `t` = every block column's true
residual ratio t_j / rtol, `mu` / `mu_prev` (the stagnation comparison), `pivots` = (kept, dropped) of the start's pivoted
Cholesky where it ran, and `steps` = one dict per step with `rank`, `pivots` = the (kept, dropped) pairs of the step's one or
two pivoted factorizations, `ratio` = max_j rel_j / rtol (where the step got that far) and `ortho` = the largest
|Q^H Q - I| over the stored stack after the step."""
import numpy as np
import scipy.sparse as sp

from blockcg_util import (DEFTOL, WIDTHS, CUTS, _herm, _select, _tri_inv, columns, deflation_batch, pchol,  # noqa: F401
                          rank_loss_case, tiny_case)
from lockstep_edges_util import CONFIG, Filtered, diagonal_levels, pair  # noqa: F401

RESTART = 10


def _norms(R):
    with np.errstate(all="ignore"):
        return np.sqrt(np.array([np.vdot(R[:, j], R[:, j]).real for j in range(R.shape[1])]))


def _tile(solve, A, B, restart, rtol, maxit, deftol, T):
    n, s = B.shape
    X = np.zeros_like(B)
    flags = np.zeros(s, dtype=np.int32)
    iters = np.zeros(s, dtype=np.int32)
    with np.errstate(all="ignore"):
        beta2 = np.array([np.vdot(B[:, j], B[:, j]).real for j in range(s)])
    excl = ~np.isfinite(beta2)
    inb = ~((beta2 == 0.0) | excl)
    flags[excl] = 1
    beta = np.sqrt(np.where(inb, beta2, 1.0))
    betaeff = np.where(inb, beta, 0.0)
    Bz = np.where(inb[None, :], B, 0.0)  # (an excluded column enters as an exact zero)
    ranks = [0, 0]
    steps, mu_prev = 0, np.inf
    t = np.full(s, np.inf)

    def end(miss):
        flags[inb] = np.where(t[inb] <= rtol, 0, miss)
        iters[inb] = steps

    if not inb.any():
        return X, flags, iters, ranks
    for c in range(10 ** 9):
        R = Bz - A @ X if c else Bz.copy()
        rho = np.where(inb, _norms(R), 0.0)
        t = np.where(inb, rho / beta, 0.0)
        mu = float(t.max())
        cyc = dict(t=(t[inb] / rtol).tolist(), mu=mu, mu_prev=mu_prev, steps=[])
        T["cycles"].append(cyc)
        if (t <= rtol).all():
            end(0)
            break
        if steps == maxit:
            end(2)
            break
        if c > 0 and not (mu < mu_prev):
            end(1)
            break
        mu_prev = mu
        live = inb & (rho != 0.0)
        Rn = np.zeros_like(R)
        Rn[:, live] = R[:, live] / rho[live]
        S, piv, r, bad, kept, dropped = pchol(_herm(Rn.conj().T @ Rn), deftol)
        cyc["pivots"] = (kept, dropped)
        if c == 0:
            ranks[0] = ranks[1] = r
        if bad or r == 0:
            end(1)
            break
        Rh = Rn @ _select(S, piv, s)
        C = S * np.where(live, rho / beta, 0.0)[None, :]
        Qs, Ps = [], []
        for j in range(restart):
            ranks[1] = r
            st = dict(rank=r, pivots=[])
            cyc["steps"].append(st)
            Z = np.stack([solve(Rh[:, i].copy()) for i in range(r)], axis=1)
            W = A @ Z
            steps += 1
            Cs = [Q.conj().T @ W for Q in Qs]
            for Q, P, Ci in zip(Qs, Ps, Cs):
                W = W - Q @ Ci
                Z = Z - P @ Ci
            S1, piv1, q, bad, kept, dropped = pchol(_herm(W.conj().T @ W), deftol)
            st["pivots"].append((kept, dropped))
            if bad:
                end(1)
                return X, flags, iters, ranks
            if q == 0:
                break
            E = _select(S1, piv1, r)
            Qj, Pj = W @ E, Z @ E
            Qs.append(Qj)
            Ps.append(Pj)
            D = Qj.conj().T @ Rh
            X = X + Pj @ ((D @ C) * betaeff[None, :])
            Rh = Rh - Qj @ D
            H = _herm(Rh.conj().T @ Rh)
            rel = np.array([np.sqrt(max(0.0, np.vdot(C[:, i], H @ C[:, i]).real)) for i in range(s)])
            st["ratio"] = float(rel.max() / rtol)
            Qall = np.concatenate(Qs, axis=1)
            st["ortho"] = float(np.abs(Qall.conj().T @ Qall - np.eye(Qall.shape[1])).max())
            if (rel <= rtol).all() or steps == maxit or j == restart - 1:
                break
            S, piv, r1, bad, kept, dropped = pchol(H, deftol)
            st["pivots"].append((kept, dropped))
            if bad:
                end(1)
                return X, flags, iters, ranks
            if r1 == 0:
                break
            Rh, C, r = Rh @ _select(S, piv, r), S @ C, r1
    return X, flags, iters, ranks


def bgcr_restated(solve, A, B, block, restart, rtol, maxit, deftol=DEFTOL, trace=None):
    """-> (X, flags, iters, ranks): the batch cut every `block` columns, every tile on its own; ranks holds each tile's rank
    after the start of its first cycle and during its last step.  solve(r) is M^{-1} r (filtered where the handle filters)."""
    solve = getattr(solve, "solve", solve)
    one = B.ndim == 1
    B = B.reshape(B.shape[0], -1)
    X = np.zeros_like(B)
    flags = np.zeros(B.shape[1], dtype=np.int32)
    iters = np.zeros(B.shape[1], dtype=np.int32)
    ranks = []
    for c0 in range(0, B.shape[1], block):
        T = dict(cycles=[])
        if trace is not None:
            trace.append(T)
        sl = slice(c0, min(c0 + block, B.shape[1]))
        X[:, sl], flags[sl], iters[sl], rk = _tile(solve, A, B[:, sl], restart, rtol, maxit, deftol, T)
        ranks += rk
    return (X[:, 0] if one else X), flags, iters, np.array(ranks, dtype=np.int32)


def decisions_ok(trace, margin):
    """every stopping ratio outside [1 / margin, margin] (each block column's t_j / rtol at every cycle start, the largest
    rel / rtol of every step), the stagnation comparison mu / mu_prev outside it too, every kept pivot >= 1e-6 and every
    dropped one <= 1e-16 in absolute value"""
    def near(v):
        return 1.0 / margin <= v <= margin

    for T in trace:
        for cyc in T["cycles"]:
            if any(near(v) for v in cyc["t"]):
                return False
            if np.isfinite(cyc["mu_prev"]) and cyc["mu_prev"] > 0 and near(cyc["mu"] / cyc["mu_prev"]):
                return False
            pivots = [cyc["pivots"]] if "pivots" in cyc else []
            for st in cyc["steps"]:
                if "ratio" in st and near(st["ratio"]):
                    return False
                pivots += st["pivots"]
            if any(k < 1e-6 or abs(d) > 1e-16 for k, d in pivots):
                return False
    return True


def summary(trace):
    """(cycles, steps, largest |Q^H Q - I|) over a trace"""
    cyc = sum(len(T["cycles"]) for T in trace)
    st = [s for T in trace for c in T["cycles"] for s in c["steps"]]
    return cyc, len(st), max([s.get("ortho", 0.0) for s in st], default=0.0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
MAXIT = 300
STAG = dict(rtol=1e-17, restart=5, width=16)


def cd48():
    """the perturbed cd2d_48 pair of the lock-step edge tests (nonsymmetric, rtol 1e-10, n = 2304)"""
    return pair("bicgstab", "cd2d_48")


def young():
    """the perturbed complex young1c pair (rtol 1e-9)"""
    return pair("bicgstab", "young1c")


def nonsym_rank_loss_case():
    """rank_loss_case with the entry (0, 5) added to its diagonal matrix: nonsymmetric, and span{e_0, e_5} is still mapped
    into itself, so the block loses two directions inside its first step -> (levels, A, B)"""
    levels, A, B = rank_loss_case()
    A = sp.lil_matrix(A)
    A[0, 5] = 0.75
    A = sp.csr_matrix(A)
    A.sort_indices()
    return levels, A, B


def filtered_pair():
    return pair("pcg", "neu2d_32_symm")


def gpu_inputs():
    """every (name, solve, A, B, block, restart, rtol, maxit) that test_gpu_blockgcr.py holds against the restatement"""
    from krylov_edges_util import neighbours_replaced
    from util import load_hier
    from oracle import orc

    P = cd48()
    n, rt = P.A.shape[0], P.rtol
    out = [("width%d" % w, P.apply, P.A, columns(n, w), w, RESTART, rt, MAXIT) for w in WIDTHS]
    out += [("cut%d_%d" % c, P.apply, P.A, columns(n, c[0]), c[1], RESTART, rt, MAXIT) for c in CUTS]
    B17 = columns(n, 17)
    # (short restarts: see test_blockgcr_host.py for why restart 1 is capped by maxit and 2, 3 stop at 1e-5)
    out.append(("restart1", P.apply, P.A, B17, 17, 1, rt, 5))
    out += [("restart%d" % m, P.apply, P.A, B17, 17, m, 1e-5, MAXIT) for m in (2, 3)]
    out.append(("restart_long", P.apply, P.A, B17, 17, 40, rt, MAXIT))
    out.append(("restart_exact", P.apply, P.A, B17, 17, ONE_CYCLE_STEPS, rt, MAXIT))
    out += [("maxit%d" % k, P.apply, P.A, columns(n, 16), 16, 5, rt, k) for k in (10, 11, 3)]
    out.append(("deflation", P.apply, P.A, deflation_batch(n, seed=DEFLATION_SEED), 8, 20, rt, MAXIT))
    levels, A, B = nonsym_rank_loss_case()
    out.append(("rank_loss", lambda r: r, A, B, 5, 64, rt, MAXIT))
    levels, A, B = tiny_case()
    out.append(("tiny", lambda r: r, A, B, 5, RESTART, rt, MAXIT))
    out.append(("stagnation", P.apply, P.A, columns(n, STAG["width"]), STAG["width"], STAG["restart"], STAG["rtol"], MAXIT))
    out.append(("excluded", P.apply, P.A, neighbours_replaced(columns(n, 5), 2, "zero"), 5, RESTART, rt, MAXIT))
    l30, d30 = load_hier("p2d_30")
    A30 = sp.csr_matrix((d30["A_vals"], d30["A_indices"], d30["A_indptr"]), shape=(len(d30["A_indptr"]) - 1,) * 2)
    out.append(("qrcp", orc.Oracle(l30), A30, columns(A30.shape[0], 5, seed=43), 5, RESTART, 1e-10, MAXIT))
    out.append(("same_bits", P.apply, P.A, columns(n, 40), 16, RESTART, rt, MAXIT))
    out.append(("vector", P.apply, P.A, columns(n, 40)[:, 3:4].copy(), 1, RESTART, rt, MAXIT))
    Y = young()
    ny = Y.A.shape[0]
    Bz = columns(ny, 5, seed=59, cplx=True)
    Bz[:, 3] = 0.0
    out.append(("complex5", Y.apply, Y.A, Bz, 5, RESTART, Y.rtol, MAXIT))
    out.append(("complex33", Y.apply, Y.A, columns(ny, 33, seed=60, cplx=True), 33, RESTART, Y.rtol, MAXIT))
    F = filtered_pair()
    out.append(("filtered", Filtered(F.O, F.Q), F.A, F.apply.proj(columns(F.A.shape[0], 33, seed=67)), 33, RESTART, F.rtol, MAXIT))
    return out


DEFLATION_SEED = 87  # (the one of 46 .. 119 whose start leaves no leftover pivot above 1e-16; test_blockgcr_host.py)
ONE_CYCLE_STEPS = 11  # the steps of the 17-column solve in one cycle (test_blockgcr_host.py asserts it)

_REF = {}


def reference(name):
    """-> ((solve, A, B, block, restart, rtol, maxit), (X, flags, iters, ranks)) of one of gpu_inputs(), restated once"""
    if "inputs" not in _REF:
        _REF["inputs"] = {i[0]: i[1:] for i in gpu_inputs()}
    if name not in _REF:
        solve, A, B, block, restart, rtol, maxit = _REF["inputs"][name]
        _REF[name] = bgcr_restated(solve, A, B, block, restart, rtol, maxit)
    return _REF["inputs"][name], _REF[name]
