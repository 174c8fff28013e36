"""Development measurement: IDR(s), s = 2, 4, 8, next to BiCGSTAB and GMRES(30) on the bench workload (the 1000^2
Poisson matrix) and on a convection-dominated matrix of the same size (upwind convection-diffusion, make_golden.convdiff2d's
generator with eps = 2e-4: the convection terms are five times the diffusion terms at h = 1 / 1001), both factorized with default
parameters by the compiled reference, 64 columns, device-pointer (torch) entries, one handle and one process per workload.

  python tests/dev_idrs.py [--out DIR] [--only poisson|convdiff]   memory, ms per step, steps and ms to 1e-8 -> DIR/idrs_krylov.json
  python tests/dev_idrs.py --trace-steps K [--s S]                 one K-step IDR(S) call after a warm-up, for a
                                                                   rocprofv3 --kernel-trace --stats run of its own
  python tests/dev_idrs.py --kernel-stats CSV                      each new kernel's time and bytes/s from the stats CSV of that
                                                                   run (bytes from the shapes: n = 10^6 rows, 64 columns, 8 B)
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NC = 1000, 64
N = NX * NX
VEC = N * NC * 8


def convdiff2d(nx, eps):
    """-eps Lap + (1, 0.5) . grad, first-order upwind (tests/golden/make_golden.py convdiff2d)"""
    h = 1.0 / (nx + 1)
    I = sp.identity(nx, format="csr")
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx), format="csr") * (eps / h / h)
    D = sp.diags([-1.0, 1.0], [-1, 0], shape=(nx, nx), format="csr") / h
    A = (sp.kron(I, T + 1.0 * D) + sp.kron(T + 0.5 * D, I)).tocsr()
    A.sort_indices()
    return A


def setup(which):
    import hifir_amd
    from oracle import ref
    from util import poisson2d

    A = poisson2d(NX) if which == "poisson" else convdiff2d(NX, 2e-4)
    t0 = time.perf_counter()
    R = ref.RefHIF(A.indptr, A.indices, A.data)
    levels = R.levels()
    print(which, "factorized in %.1f s, %d levels" % (time.perf_counter() - t0, len(levels)), flush=True)
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
    M.set_matrix(A.indptr, A.indices, A.data)
    return A, M


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure_one(which):
    import torch

    A, M = setup(which)
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()
    Bh = B.cpu().numpy()
    bn = np.linalg.norm(Bh, axis=0)
    res = {"n": N, "nrhs": NC}

    def mem_first(fn):
        torch.cuda.synchronize()
        f0 = torch.cuda.mem_get_info()[0]
        out = fn()
        torch.cuda.synchronize()
        return f0 - torch.cuda.mem_get_info()[0], out

    def to_tol(fn):
        ms, (X, fl, it) = timed(fn)
        rr = np.linalg.norm(A @ X.cpu().numpy() - Bh, axis=0) / bn
        del X
        return {"ms": ms, "flags": sorted(set(fl.tolist())), "steps_min_mean_max": [int(it.min()), float(it.mean()), int(it.max())],
                "true_relres_max": float(rr.max())}

    # (IDR(4) first: what its first call takes on a handle that has run no solver yet)
    for s in (4, 2, 8):
        taken, _ = mem_first(lambda: M.idrs(B, s=s, rtol=1e-300, maxit=2))
        res["idrs%d_first_call_bytes" % s] = int(taken)  # (s = 2: nothing new; s = 8: what it adds to s = 4's)
        t18, _ = timed(lambda: M.idrs(B, s=s, rtol=1e-300, maxit=18))
        t36, (_, f36, _) = timed(lambda: M.idrs(B, s=s, rtol=1e-300, maxit=36))
        res["idrs%d_ms_per_step" % s] = (t36 - t18) / 18
        res["idrs%d_t18_t36_ms" % s] = [t18, t36]
        res["idrs%d_maxit36_flags" % s] = sorted(set(f36.tolist()))
        res["idrs%d_to_1e-8" % s] = to_tol(lambda: M.idrs(B, s=s, rtol=1e-8, maxit=1000))
        print(which, "IDR(%d)" % s, res["idrs%d_ms_per_step" % s], res["idrs%d_to_1e-8" % s], flush=True)
    M.bicgstab(B, rtol=1e-300, maxit=2)
    t20, _ = timed(lambda: M.bicgstab(B, rtol=1e-300, maxit=20))
    t40, (_, f40, _) = timed(lambda: M.bicgstab(B, rtol=1e-300, maxit=40))
    res["bicgstab_ms_per_step"] = (t40 - t20) / 20
    res["bicgstab_maxit40_flags"] = sorted(set(f40.tolist()))
    res["bicgstab_to_1e-8"] = to_tol(lambda: M.bicgstab(B, rtol=1e-8, maxit=1000))
    print(which, "BiCGSTAB", res["bicgstab_ms_per_step"], res["bicgstab_to_1e-8"], flush=True)
    taken, _ = mem_first(lambda: M.gmres(B, restart=30, rtol=1e-300, maxit=2))
    res["gmres30_first_call_bytes_after_idrs"] = int(taken)
    t1, _ = timed(lambda: M.gmres(B, restart=30, rtol=1e-300, maxit=1))
    t30, _ = timed(lambda: M.gmres(B, restart=30, rtol=1e-300, maxit=30))
    res["gmres30_ms_per_inner_step"] = (t30 - t1) / 29
    res["gmres30_to_1e-8"] = to_tol(lambda: M.gmres(B, restart=30, rtol=1e-8, maxit=1000))
    print(which, "GMRES(30)", res["gmres30_ms_per_inner_step"], res["gmres30_to_1e-8"], flush=True)
    M.close()
    return res


def measure(out_dir, only):
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "idrs_krylov.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    res["workloads"] = {"poisson": "poisson2d(1000), default parameters, 64 columns, torch-device entries",
                        "convdiff": "convdiff2d(1000, eps = 2e-4), default parameters, 64 columns, torch-device entries"}
    for which in ("poisson", "convdiff"):
        if only in (None, which):
            res[which] = measure_one(which)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def trace(steps, s):
    import torch

    A, M = setup("poisson")
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()
    M.idrs(B, s=s, rtol=1e-300, maxit=2)  # warm-up: buffers and the apply's graph
    torch.cuda.synchronize()
    _, fl, it = M.idrs(B, s=s, rtol=1e-300, maxit=steps)
    torch.cuda.synchronize()
    print("trace IDR(%d)" % s, steps, "steps:", sorted(set(it.tolist())))


def kernel_vecs(name):
    """vectors of [n][64] float64 a kernel reads plus writes, from its template arguments"""
    m = re.search(r"k_idr_comb<\w+, (\d+), \w+>", name)
    if m:
        return int(m.group(1)) + 2  # the run, z, y
    m = re.search(r"k_idr_gu<\w+, (\d+)>", name)
    if m:
        S = int(m.group(1))
        return 2 * S + (8 if S else 6)  # the two runs, g_k, u_k, r, x read; r, x (and g_k, u_k when S > 0) written
    if "k_idr_finish" in name:
        return 0
    if "k_nsp_coef" in name:
        return 1
    return None


def kernel_stats(path):
    out = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        nv = kernel_vecs(name)
        if nv is None:
            continue
        short = re.search(r"(k_\w+<[^>]*>)", name).group(1)
        avg_ns = float(r["AverageNs"])
        out[short] = {"calls": int(r["Calls"]), "avg_us": avg_ns / 1e3, "bytes": nv * VEC, "GB_per_s": (nv * VEC / avg_ns) if nv else None}
    print(json.dumps(out, indent=1))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", choices=["poisson", "convdiff"])
    ap.add_argument("--trace-steps", type=int)
    ap.add_argument("--s", type=int, default=4)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats)
    elif a.trace_steps:
        trace(a.trace_steps, a.s)
    else:
        measure(a.out or ".", a.only)
