#!/usr/bin/env python3
"""Regenerates the two Hermitian INDEFINITE fixtures of the symmetric QMR driver (tests/golden/hier_<name>.npz) from the
REAL reference; needs what make_golden.py needs (the compiled reference, `make -C oracle ref`).

Each file holds what make_golden.save_hier stores (the hierarchy field by field, the matrix, b, ...).

  shift2d_32_symm  poisson2d(32) - 0.30 I: 1,024 rows, 20 negative eigenvalues, smallest |lambda| 3.3e-3
  kktr_24_symm     [[K, B^T], [B, 0]], K = poisson2d(24), B 150 x 576 with three entries per row i = 0 ... 149:
                   B[i, 3i] = 1, B[i, (7i + 5) mod 576] = 0.5, B[i, (11i + 2) mod 576] = -0.5: a real saddle-point
                   (KKT) system of 726 rows with 150 negative eigenvalues, smallest |lambda| 0.13
both factorized with is_symm = 1, tau = 1e-2, kappa = 5, alpha = 3, dense_thres = 60: two sparse levels and a SYEIG
block each, M^{-1} Hermitian (mirrored bit for bit) and indefinite.
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import poisson2d, ref, save_hier  # noqa: E402


def shifted_poisson(nx, shift=0.30):
    A = (poisson2d(nx) - shift * sp.identity(nx * nx, format="csr")).tocsr()
    A.sort_indices()
    return A


def real_kkt(nx=24, nb=150):
    K = poisson2d(nx)
    nk = nx * nx
    i = np.arange(nb)
    rows = np.concatenate([i, i, i])
    cols = np.concatenate([3 * i, (7 * i + 5) % nk, (11 * i + 2) % nk])
    vals = np.concatenate([np.ones(nb), 0.5 * np.ones(nb), -0.5 * np.ones(nb)])
    B = sp.csr_matrix((vals, (rows, cols)), shape=(nb, nk))
    A = sp.bmat([[K, B.T], [B, None]], format="csr")
    A.sort_indices()
    return A


def report(name, A):
    w = np.linalg.eigvalsh(A.toarray())
    path = os.path.join(HERE, f"hier_{name}.npz")
    print(f"hier_{name}.npz: n={A.shape[0]} negative eigenvalues={int((w < 0).sum())} min|lambda|={np.abs(w).min():.2e} "
          f"size={os.path.getsize(path) / 1e6:.2f} MB")


def main():
    params = ref.make_params(is_symm=1, tau=1e-2, kappa=5.0, alpha=3.0, dense_thres=60)
    for name, A in (("shift2d_32_symm", shifted_poisson(32)), ("kktr_24_symm", real_kkt())):
        save_hier(name, A, params)
        report(name, A)


if __name__ == "__main__":
    main()
