"""Inputs and restatements for the extra-precise residual, the refinement under it and GMRES-IR (test_xp_resid_host.py pins
them on the CPU, test_gpu_xp_resid.py holds the kernel and the drivers against them).  numpy / scipy / fractions only.

resid_dd restates k_crs_resid_dd operation for operation, vectorized over the columns of a batch: the device
result has to equal it bit for bit.  TwoProd's error term comes from math.fma where Python has it and from Dekker's product
(Veltkamp split at 27 bits) otherwise; both are exact barring over- and underflow, so the bits agree for the magnitudes used
here.  resid_working restates k_crs_spmm<T, true> the same way; resid_exact is the rational residual.

The hard inputs are dense graded matrices with entries rounded to float32 and right-hand sides b = A xt for small integer xt:
b is exact (asserted with Fraction), so xt IS the solution and a forward error of eps is a meaningful bar."""
import functools
import math
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

from dense_level_util import dense_level

EPS = 2.0 ** -53
_FMA = getattr(math, "fma", None)


# ---- error-free transformations -------------------------------------------------------------------------------------------
def _split(v):
    c = 134217729.0 * v  # 2^27 + 1
    h = c - (c - v)
    return h, v - h


def two_prod_err(a, x, p):
    """e with a * x = p + e exactly (p = fl(a * x)); a scalar, x and p vectors"""
    if _FMA is not None:
        return np.array([_FMA(a, float(xi), -float(pi)) for xi, pi in zip(x, p)])
    ah, al = _split(np.float64(a))
    xh, xl = _split(x)
    return ((ah * xh - p) + ah * xl + al * xh) + al * xl


def dd_step(s, c, a, x):
    """one nonzero of the compensated sum, with the coefficient a as the kernel passes it (already signed)"""
    p = a * x
    e = two_prod_err(a, x, p)
    t = s + p
    z = t - s
    q = (s - (t - z)) + (p - z)
    return t, c + (q + e)


def _block(V):
    V = np.asarray(V)
    return V.reshape(V.shape[0], -1)


def resid_dd(indptr, indices, vals, B, X):
    """B - A X as k_crs_resid_dd forms it; B, X (n,) or (n, k)"""
    B2, X2 = _block(B), _block(X)
    cplx = np.iscomplexobj(vals) or np.iscomplexobj(B2) or np.iscomplexobj(X2)
    n = len(indptr) - 1
    R = np.empty(B2.shape, dtype=np.complex128 if cplx else np.float64)
    with np.errstate(all="ignore"):
        for i in range(n):
            if not cplx:
                s, c = B2[i].astype(np.float64), np.zeros(B2.shape[1])
                for k in range(indptr[i], indptr[i + 1]):
                    s, c = dd_step(s, c, -float(vals[k]), X2[indices[k]])
                R[i] = s + c
                continue
            b = B2[i].astype(np.complex128)
            sr, cr, si, ci = b.real.copy(), np.zeros(B2.shape[1]), b.imag.copy(), np.zeros(B2.shape[1])
            for k in range(indptr[i], indptr[i + 1]):
                a = complex(vals[k])
                x = X2[indices[k]].astype(np.complex128)
                xr, xi = x.real.copy(), x.imag.copy()
                sr, cr = dd_step(sr, cr, -a.real, xr)
                sr, cr = dd_step(sr, cr, a.imag, xi)
                si, ci = dd_step(si, ci, -a.real, xi)
                si, ci = dd_step(si, ci, -a.imag, xr)
            R[i] = (sr + cr) + 1j * (si + ci)
    return R.reshape(np.asarray(B).shape)


def resid_working(indptr, indices, vals, B, X):
    """B - A X as k_crs_spmm<T, true> forms it: tmp = 0; tmp += a * x in CRS order; b - tmp (complex products spelled out,
    every operation rounded on its own)"""
    B2, X2 = _block(B), _block(X)
    cplx = np.iscomplexobj(vals) or np.iscomplexobj(B2) or np.iscomplexobj(X2)
    n = len(indptr) - 1
    R = np.empty(B2.shape, dtype=np.complex128 if cplx else np.float64)
    with np.errstate(all="ignore"):
        for i in range(n):
            if not cplx:
                acc = np.zeros(B2.shape[1])
                for k in range(indptr[i], indptr[i + 1]):
                    acc = acc + float(vals[k]) * X2[indices[k]]
                R[i] = B2[i] - acc
                continue
            ar_, ai_ = np.zeros(B2.shape[1]), np.zeros(B2.shape[1])
            for k in range(indptr[i], indptr[i + 1]):
                a = complex(vals[k])
                x = X2[indices[k]].astype(np.complex128)
                xr, xi = x.real.copy(), x.imag.copy()
                ar_ = ar_ + (a.real * xr - a.imag * xi)
                ai_ = ai_ + (a.real * xi + a.imag * xr)
            b = B2[i].astype(np.complex128)
            R[i] = (b.real - ar_) + 1j * (b.imag - ai_)
    return R.reshape(np.asarray(B).shape)


def _frac(v):
    return Fraction(float(v))


def resid_exact(indptr, indices, vals, b, x):
    """the exact residual of ONE column: a list of Fraction (real) or of (Fraction, Fraction) pairs (complex)"""
    cplx = np.iscomplexobj(vals) or np.iscomplexobj(b) or np.iscomplexobj(x)
    out = []
    for i in range(len(indptr) - 1):
        if not cplx:
            r = _frac(b[i])
            for k in range(indptr[i], indptr[i + 1]):
                r -= _frac(vals[k]) * _frac(x[indices[k]])
            out.append(r)
            continue
        bi = complex(b[i])
        rr, ri = _frac(bi.real), _frac(bi.imag)
        for k in range(indptr[i], indptr[i + 1]):
            a, xv = complex(vals[k]), complex(x[indices[k]])
            ar, ai, xr, xi = _frac(a.real), _frac(a.imag), _frac(xv.real), _frac(xv.imag)
            rr -= ar * xr - ai * xi
            ri -= ar * xi + ai * xr
        out.append((rr, ri))
    return out


def exact_norm(r):
    """2-norm of resid_exact's list, as a float"""
    tot = Fraction(0)
    for v in r:
        tot += v[0] * v[0] + v[1] * v[1] if isinstance(v, tuple) else v * v
    return math.sqrt(tot)


def dot2_bound(indptr, indices, vals, b, x, r_exact):
    """Per row, the bound of Ogita, Rump and Oishi for the compensated dot product with b_i as the first term:
    eps |r| + gamma_m^2 (|b_i| + sum |a||x|), gamma_m = m eps / (1 - m eps), m = terms + 1 (a complex nonzero is two terms of
    each part; the magnitudes of a complex row are bounded with |Re| + |Im|)"""
    cplx = isinstance(r_exact[0], tuple)
    out = []
    for i in range(len(indptr) - 1):
        nz = int(indptr[i + 1] - indptr[i])
        m = (2 * nz if cplx else nz) + 1
        g = m * EPS / (1 - m * EPS)
        if cplx:
            mag = abs(complex(b[i]).real) + abs(complex(b[i]).imag)
            for k in range(indptr[i], indptr[i + 1]):
                a, xv = complex(vals[k]), complex(x[indices[k]])
                mag += (abs(a.real) + abs(a.imag)) * (abs(xv.real) + abs(xv.imag))
            rm = max(abs(float(r_exact[i][0])), abs(float(r_exact[i][1])))
        else:
            mag = abs(float(b[i]))
            for k in range(indptr[i], indptr[i + 1]):
                mag += abs(float(vals[k])) * abs(float(x[indices[k]]))
            rm = abs(float(r_exact[i]))
        out.append(EPS * rm + g * g * mag)
    return np.array(out)


def err_vs_exact(r, r_exact):
    """per row |r - r_exact| (complex: the larger of the two parts), computed exactly and rounded once"""
    out = []
    for v, e in zip(r, r_exact):
        if isinstance(e, tuple):
            v = complex(v)
            out.append(max(abs(float(_frac(v.real) - e[0])), abs(float(_frac(v.imag) - e[1]))))
        else:
            out.append(abs(float(_frac(v) - e)))
    return np.array(out)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
GRADED = ((48, 1e9, 11), (130, 1e10, 12))  # (rows, kappa asked for, seed); the host test pins the condition numbers
RTOL_FWD = 1e-27  # eps / cond(A) for cond(A) <= 1e11: the residual that bounds the forward error by eps
NCOLS = 5  # right-hand sides of a graded case, each with its own xt (the GPU tests add a zero column)


def _orth(rng, n, cplx):
    G = rng.normal(size=(n, n))
    if cplx:
        G = G + 1j * rng.normal(size=(n, n))
    return np.linalg.qr(G)[0]


def graded(n, kappa, seed, cplx=False):
    """U diag(logspace(0, -log10 kappa)) V^H rounded to float32 and widened, as a dense-pattern CRS:
    (indptr int64, indices int32, vals, dense)"""
    rng = np.random.default_rng(seed)
    U, V = _orth(rng, n, cplx), _orth(rng, n, cplx)
    A = (U * np.logspace(0, -np.log10(kappa), n)) @ V.conj().T
    if cplx:
        A = A.real.astype(np.float32).astype(np.float64) + 1j * A.imag.astype(np.float32).astype(np.float64)
    else:
        A = A.astype(np.float32).astype(np.float64)
    indptr = np.arange(0, n * n + 1, n, dtype=np.int64)
    indices = np.tile(np.arange(n, dtype=np.int32), n)
    return indptr, indices, A.ravel().copy(), A


def int_solution(rng, shape, cplx=False):
    """nonzero integers in +-[1, 8]"""
    def draw():
        return rng.integers(1, 9, size=shape) * rng.choice([-1, 1], size=shape)
    return (draw() + 1j * draw()).astype(np.complex128) if cplx else draw().astype(np.float64)


def exact_rhs(indptr, indices, vals, xt):
    """b = A xt, asserted exact: every entry's rational value is a double"""
    xt2 = _block(xt)
    B = np.empty(xt2.shape, dtype=xt2.dtype if np.iscomplexobj(xt2) or not np.iscomplexobj(vals) else np.complex128)
    zero = np.zeros(xt2.shape[0], dtype=B.dtype)
    for c in range(xt2.shape[1]):
        r = resid_exact(indptr, indices, vals, zero, xt2[:, c])
        for i, v in enumerate(r):
            if isinstance(v, tuple):
                re, im = float(-v[0]), float(-v[1])
                assert Fraction(re) == -v[0] and Fraction(im) == -v[1], "b = A xt is not exact"
                B[i, c] = re + 1j * im
            else:
                f = float(-v)
                assert Fraction(f) == -v, "b = A xt is not exact"
                B[i, c] = f
    return B.reshape(np.asarray(xt).shape)


@functools.lru_cache(maxsize=None)
def graded_case(which, cplx):
    """(computed once, shared, never written to) -> dict(n, indptr, indices, vals, A, XT (n, NCOLS), B = A XT exact)"""
    n, kappa, seed = GRADED[which]
    indptr, indices, vals, A = graded(n, kappa, seed, cplx)
    XT = int_solution(np.random.default_rng(1000 + seed), (n, NCOLS), cplx)
    return dict(n=n, indptr=indptr, indices=indices, vals=vals, A=A, XT=XT, B=exact_rhs(indptr, indices, vals, XT))


FIXTURES = ("p2d_30", "pcd2d_32", "young1c")  # fixtures that carry their matrix (young1c: complex)


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """(computed once, shared, never written to) -> dict(levels, n, indptr, indices, vals, XT (n, 3) integer, B = A XT
    in working precision: a right-hand side like any other, the checks on these are residual checks)"""
    from util import load_hier

    levels, d = load_hier(name)
    n = len(d["b"])
    A = sp.csr_matrix((d["A_vals"], d["A_indices"], d["A_indptr"]), shape=(n, n))
    A.sort_indices()
    XT = int_solution(np.random.default_rng(77), (n, 3), np.iscomplexobj(A.data))
    return dict(levels=levels, n=n, indptr=A.indptr.astype(np.int64), indices=A.indices.astype(np.int32), vals=A.data.copy(),
                A=A, XT=XT, B=np.ascontiguousarray(A @ XT))


def adjoint_crs(indptr, indices, vals, n):
    """the conjugate transpose as a CRS with sorted rows (what adjoint_of_csr builds on the host)"""
    At = sp.csr_matrix((vals, indices, indptr), shape=(n, n)).conj().T.tocsr()
    At.sort_indices()
    return At.indptr.astype(np.int64), At.indices.astype(np.int32), At.data.copy()


def one_level(A):
    """A one-level hierarchy with M = A: no sparse rows, unit scalings, identity permutations, the dense block A handed
    over as a QRCP block (the drivers are then run at full rank: the numerical rank rule cuts near 1 / eps^(2/3) ~ 2.7e10,
    where the larger graded matrix sits)."""
    n = A.shape[0]
    dtype = np.complex128 if np.iscomplexobj(A) else np.float64
    lv = dense_level(n, "qrcp", dtype, m=0, seed=1)[0]
    lv["s"], lv["t"] = np.ones(n), np.ones(n)
    for k in ("p", "q", "p_inv", "q_inv"):
        lv[k] = np.arange(n, dtype=np.int32)
    lv["dense"] = np.asarray(A, dtype=dtype).ravel(order="F").copy()
    return [lv]


def fwd_ok(X, XT):
    """|x - xt| <= 2 eps |xt| componentwise"""
    return bool(np.all(np.abs(X - XT) <= 2 * EPS * np.abs(XT)))


def fwd_err(X, XT):
    return float(np.max(np.abs(X - XT) / np.abs(XT)))


# ---- the drivers restated -------------------------------------------------------------------------------------------------
def refine(solve, resid, b, sweeps):
    """x = 0; per sweep x += M^-1 (b - A x) (the first residual is b); -> the iterate after every sweep"""
    x = np.zeros_like(b)
    out = []
    for i in range(sweeps):
        r = resid(b, x) if i else b.copy()
        x = x + solve(r)
        out.append(x.copy())
    return out


def gmres_1col(matvec, solve, b, restart, rtol, maxit):
    """right-preconditioned restarted GMRES for one column (x0 = 0, modified Gram-Schmidt, least squares by lstsq):
    -> (x, iterations)"""
    n = len(b)
    x = np.zeros_like(b)
    bn = np.linalg.norm(b)
    if bn == 0:
        return x, 0
    its = 0
    while its < maxit:
        r = b - matvec(x) if its else b.copy()
        beta = np.linalg.norm(r)
        if beta / bn <= rtol:
            break
        Q = np.zeros((n, restart + 1), dtype=b.dtype)
        Z = np.zeros((n, restart), dtype=b.dtype)
        H = np.zeros((restart + 1, restart), dtype=b.dtype)
        Q[:, 0] = r / beta
        y, j = None, 0
        for j in range(restart):
            Z[:, j] = solve(Q[:, j])
            w = matvec(Z[:, j])
            for i in range(j + 1):
                H[i, j] = np.vdot(Q[:, i], w)
                w = w - H[i, j] * Q[:, i]
            H[j + 1, j] = np.linalg.norm(w)
            its += 1
            e1 = np.zeros(j + 2, dtype=b.dtype)
            e1[0] = beta
            y = np.linalg.lstsq(H[:j + 2, :j + 1], e1, rcond=None)[0]
            res = np.linalg.norm(H[:j + 2, :j + 1] @ y - e1) / bn
            if res <= rtol or its >= maxit or H[j + 1, j] == 0:
                break
            Q[:, j + 1] = w / H[j + 1, j]
        x = x + Z[:, :j + 1] @ y
        if res <= rtol:
            break
    return x, its


def gmres_ir(matvec, solve, resid, b, restart=30, rtol=1e-14, inner_rtol=1e-6, max_outer=10, inner_maxit=500):
    """GMRES-IR for one column as gmres_ir_tile runs it: -> (x, flag, corrections in x, inner iterations, relres)"""
    x = np.zeros_like(b)
    bn = np.linalg.norm(b)
    if bn == 0:
        return x, 0, 0, 0, 0.0
    prev, xk, outer, iters = None, None, 0, 0
    for k in range(max_outer + 1):
        r = resid(b, x) if k else b.copy()
        res = np.linalg.norm(r) / bn
        if not np.isfinite(res) or (k > 0 and res >= prev):
            return (xk, 1, outer - 1, iters, prev) if k else (x, 1, 0, 0, res)
        if res <= rtol:
            return x, 0, outer, iters, res
        if k == max_outer:
            return x, 2, outer, iters, res
        d, it = gmres_1col(matvec, solve, r, restart, inner_rtol, inner_maxit)
        prev, xk = res, x
        x = x + d
        outer, iters = outer + 1, iters + it
    raise AssertionError("unreachable")
