"""Development measurement: symmetric QMR next to PCG, BiCGSTAB and GMRES(30), 64 columns, device-pointer
(torch) entries, hierarchies factorized with is_symm by the compiled reference.

The matrix asked for, poisson2d(1000) - 0.30 I, has no is_symm factorization to measure on: the reference turns the second
Schur complement of the shifted matrix dense (1,545 of 10,000 rows at 100^2, a SYEIG block of that share at every size
tried) and its process dies at 1000^2.  So the time and memory figures are taken where they can be, on the UNSHIFTED
1000^2 matrix (a positive-definite pair is a valid input; the passes do not depend on definiteness), with PCG and a
BiCGSTAB step on the same handle in the same process; the iteration counts of an indefinite solve come from
poisson2d(100) - 0.30 I.

  python tests/dev_sqmr.py [--out DIR]          memory, ms per iteration, iterations to 1e-8 -> DIR/sqmr_krylov.json (DIR: .)
  python tests/dev_sqmr.py --trace-iters K      one K-iteration symmetric QMR call after a warm-up, for a
                                                rocprofv3 --kernel-trace --stats run of its own
  python tests/dev_sqmr.py --kernel-stats CSV   each k_qm_* kernel's time and bytes/s from the stats CSV of that run
                                                (bytes from the shapes: n = 10^6 rows, 64 columns, 8 B)
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NC = 1000, 64
NX_INDEF, SHIFT = 100, 0.30
N = NX * NX
VEC = N * NC * 8
MAXIT = 500  # cap of the runs to rtol 1e-8
# vectors of [n][64] float64 each kernel reads plus writes
KERNEL_VECS = {"k_qm_r": 3, "k_qm_ds": 10, "k_qm_finish": 0, "k_cg_p": 3}


def setup(nx=NX, shift=0.0):
    import scipy.sparse as sp

    import hifir_amd
    from oracle import ref
    from util import poisson2d

    A = poisson2d(nx)
    if shift:
        A = (A - shift * sp.identity(nx * nx, format="csr")).tocsr()
        A.sort_indices()
    t0 = time.perf_counter()
    R = ref.RefHIF(A.indptr, A.indices, A.data, ref.make_params(is_symm=1))
    levels = R.levels()
    info = {"matrix": f"poisson2d({nx})" + (f" - {shift} I" if shift else ""), "factorize_s": time.perf_counter() - t0,
            "levels": [[int(lv["m"]), int(lv["n"])] for lv in levels], "dense_n": int(levels[-1].get("dense_n", 0))}
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=NC)
    info["hermitian"] = bool(M.is_hermitian())
    M.set_matrix(A.indptr, A.indices, A.data)
    return A, M, info


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _counts(it):
    return [int(it.min()), float(it.mean()), int(it.max())]


def per_iteration(solver, B, lo, hi):
    """(t_hi - t_lo) / (hi - lo) with rtol out of reach, and what the two calls returned"""
    solver(B, rtol=1e-300, maxit=2)  # warm-up: buffers and the apply's graph
    t_lo, (_, f_lo, i_lo) = timed(lambda: solver(B, rtol=1e-300, maxit=lo))
    t_hi, (_, f_hi, i_hi) = timed(lambda: solver(B, rtol=1e-300, maxit=hi))
    full = bool((i_lo == lo).all() and (i_hi == hi).all())
    return {"ms_per_iteration": (t_hi - t_lo) / (hi - lo) if full else None, "t_lo_hi_ms": [t_lo, t_hi], "maxit_lo_hi": [lo, hi],
            "every_column_ran_to_maxit": full, "flags_hi": sorted(set(f_hi.tolist())), "iters_hi_min_mean_max": _counts(i_hi)}


def to_tol(solver, A, B, Bh, **kw):
    ms, (X, fl, it) = timed(lambda: solver(B, rtol=1e-8, maxit=MAXIT, **kw))
    Xh = X.cpu().numpy()
    rr = np.linalg.norm(A @ Xh - Bh, axis=0) / np.linalg.norm(Bh, axis=0)
    flags = {int(f): int((fl == f).sum()) for f in sorted(set(fl.tolist()))}
    return {"ms": ms, "columns_by_flag": flags, "iters_min_mean_max": _counts(it),
            "true_relres_max_of_converged": float(rr[fl == 0].max()) if (fl == 0).any() else None,
            "true_relres_max": float(np.nanmax(rr)) if np.isfinite(rr).any() else None}


def measure(out_dir):
    import torch

    A, M, info = setup()
    res = {"workload": f"make_params(is_symm=1), {NC} columns, torch-device entries", "nrhs": NC,
           "timed": {"n": N, "hierarchy": info}}
    print(json.dumps(info), flush=True)
    assert info["hermitian"]
    T = res["timed"]
    Bh = np.random.default_rng(7).uniform(-1, 1, size=(N, NC))
    B = torch.from_numpy(Bh).cuda()
    torch.cuda.synchronize()
    f0 = torch.cuda.mem_get_info()[0]
    M.sqmr(B, rtol=1e-300, maxit=2)
    torch.cuda.synchronize()
    T["sqmr_first_call_bytes"] = int(f0 - torch.cuda.mem_get_info()[0])
    T["sqmr"] = per_iteration(M.sqmr, B, 10, 30)
    T["pcg"] = per_iteration(M.pcg, B, 10, 30)
    T["bicgstab_step"] = per_iteration(M.bicgstab, B, 20, 40)
    T["sqmr_again"] = per_iteration(M.sqmr, B, 10, 30)  # the spread of the same measurement
    print(json.dumps(res, indent=1), flush=True)
    T["sqmr_to_1e-8"] = to_tol(M.sqmr, A, B, Bh)
    T["pcg_to_1e-8"] = to_tol(M.pcg, A, B, Bh)
    T["bicgstab_to_1e-8"] = to_tol(M.bicgstab, A, B, Bh)
    T["gmres30_to_1e-8"] = to_tol(M.gmres, A, B, Bh, restart=30)
    del M, B
    # the indefinite pair, at the size its factorization exists: iteration counts only (a 10,000-row solve times overheads)
    A, M, info = setup(NX_INDEF, SHIFT)
    n = NX_INDEF * NX_INDEF
    I = res["indefinite"] = {"n": n, "hierarchy": info}
    if info["hermitian"]:
        Bh = np.random.default_rng(7).uniform(-1, 1, size=(n, NC))
        B = torch.from_numpy(Bh).cuda()
        I["sqmr_to_1e-8"] = to_tol(M.sqmr, A, B, Bh)
        I["pcg_to_1e-8"] = to_tol(M.pcg, A, B, Bh)
        I["bicgstab_to_1e-8"] = to_tol(M.bicgstab, A, B, Bh)
        I["gmres30_to_1e-8"] = to_tol(M.gmres, A, B, Bh, restart=30)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "sqmr_krylov.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def trace(iters):
    import torch

    A, M, info = setup()
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()
    M.sqmr(B, rtol=1e-300, maxit=2)  # warm-up: buffers and the apply's graph
    torch.cuda.synchronize()
    _, fl, it = M.sqmr(B, rtol=1e-300, maxit=iters)
    torch.cuda.synchronize()
    print("trace", iters, "iterations:", sorted(set(it.tolist())), "flags", sorted(set(fl.tolist())))


def kernel_stats(path):
    rows = list(csv.DictReader(open(path)))
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        for k, nv in KERNEL_VECS.items():
            if k + "<" in name or k + "(" in name or name.split("<")[0].split("(")[0].endswith(k):
                avg_ns = float(r["AverageNs"])
                out[k] = {"calls": int(r["Calls"]), "avg_us": avg_ns / 1e3,
                          "bytes": nv * VEC, "GB_per_s": (nv * VEC / avg_ns) if nv else None}
    print(json.dumps(out, indent=1))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace-iters", type=int)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats)
    elif a.trace_iters:
        trace(a.trace_iters)
    else:
        measure(a.out or ".")
