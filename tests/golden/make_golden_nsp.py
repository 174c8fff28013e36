#!/usr/bin/env python3
"""Regenerates the three singular fixtures of the basis null-space filter (tests/golden/hier_<name>.npz) from the
REAL reference; needs what make_golden.py needs (the compiled reference, `make -C oracle ref`).

Each file holds what make_golden.save_hier stores (the hierarchy field by field, the matrix, b, ...) plus
  xstar   x* uniform in (-1, 1)            bstar   A x* (a consistent right-hand side)
  V       (n, k) basis of the right null space of A        VL   (pcd2d_32 only) basis of the left null space
  x_nspc  (neu2d_32_symm only) the reference's own solve(b) with set_nsp_const(0, -1) in force

  neu2d_32_symm  5-point Laplacian of the 32 x 32 grid graph (pure Neumann), null space = constants, is_symm
  twobody_symm   blockdiag(D1 N24 D1, D2 N20 D2): two floating bodies, null space = {D1^-1 1, D2^-1 1}, is_symm
  pcd2d_32       D1 K D2, K = periodic 32 x 32 Laplacian + 0.4 / 0.2 x periodic central differences (row and column
                 sums zero), nonsymmetric: right null vector D2^-1 1, left null vector D1^-1 1
all factorized with tau = 1e-2, kappa = 5, alpha = 3, dense_thres = 60 (defaults solve these sizes in 2-3 steps).
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ref, save_hier  # noqa: E402


def neumann1d(nx):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx), format="lil")
    T[0, 0] = 1.0
    T[nx - 1, nx - 1] = 1.0
    return T.tocsr()


def neumann2d(nx):
    T = neumann1d(nx)
    I = sp.identity(nx, format="csr")
    A = (sp.kron(I, T) + sp.kron(T, I)).tocsr()
    A.sort_indices()
    return A


def scalings(n):
    i = np.arange(n)
    return 1.0 + 0.5 * np.sin(0.37 * i), 1.0 + 0.5 * np.cos(0.23 * i)


def two_body(nx, ny):
    n1, n2 = nx * nx, ny * ny
    d1, d2 = scalings(n1)[0], scalings(n2)[1]
    A = sp.block_diag([sp.diags(d1) @ neumann2d(nx) @ sp.diags(d1), sp.diags(d2) @ neumann2d(ny) @ sp.diags(d2)]).tocsr()
    A.sort_indices()
    V = np.zeros((n1 + n2, 2))
    V[:n1, 0] = 1.0 / d1
    V[n1:, 1] = 1.0 / d2
    return A, V


def periodic_cd(nx):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx), format="lil")
    T[0, nx - 1] = -1.0
    T[nx - 1, 0] = -1.0
    C = sp.diags([-1.0, 1.0], [-1, 1], shape=(nx, nx), format="lil")
    C[0, nx - 1] = -1.0
    C[nx - 1, 0] = 1.0
    T, C, I = T.tocsr(), C.tocsr(), sp.identity(nx, format="csr")
    K = sp.kron(I, T + 0.4 * C) + sp.kron(T + 0.2 * C, I)
    d1, d2 = scalings(nx * nx)
    A = (sp.diags(d1) @ K @ sp.diags(d2)).tocsr()
    A.sort_indices()
    return A, (1.0 / d2)[:, None], (1.0 / d1)[:, None]


def save_nsp(name, A, params, V, VL=None, nspc=False, seed=11):
    save_hier(name, A, params)
    path = os.path.join(HERE, f"hier_{name}.npz")
    d = dict(np.load(path))
    n = A.shape[0]
    xstar = np.random.default_rng(seed).uniform(-1.0, 1.0, n)
    d.update(xstar=xstar, bstar=A @ xstar, V=np.ascontiguousarray(V))
    if VL is not None:
        d["VL"] = np.ascontiguousarray(VL)
    if nspc:
        M = ref.RefHIF(A.indptr, A.indices, A.data.astype(np.float64), params)
        M.set_nsp_const(0, -1)
        d["x_nspc"] = M.solve(d["b"])
    np.savez_compressed(path, **d)
    scale = abs(A).max()
    print(f"hier_{name}.npz: k={V.shape[1]} |A V|/|A|={np.abs(A @ V).max() / scale:.1e}"
          + ("" if VL is None else f" |A^T VL|/|A|={np.abs(A.T @ VL).max() / scale:.1e}")
          + f" size={os.path.getsize(path) / 1e6:.2f} MB")


def main():
    kw = dict(tau=1e-2, kappa=5.0, alpha=3.0, dense_thres=60)
    A = neumann2d(32)
    save_nsp("neu2d_32_symm", A, ref.make_params(is_symm=1, **kw), np.ones((A.shape[0], 1)), nspc=True)
    A, V = two_body(24, 20)
    save_nsp("twobody_symm", A, ref.make_params(is_symm=1, **kw), V)
    A, V, VL = periodic_cd(32)
    save_nsp("pcd2d_32", A, ref.make_params(**kw), V, VL=VL)


if __name__ == "__main__":
    main()
