"""Development measurement: BiCGSTAB next to GMRES(30) on the bench workload, the 1000^2 Poisson matrix
factorized with default parameters by the compiled reference, 64 columns, device-pointer (torch) entries.

  python tests/dev_krylov.py [--out DIR]          memory, ms per step, steps and time to 1e-8 -> DIR/krylov.json (DIR: .)
  python tests/dev_krylov.py --trace-steps K      one K-step BiCGSTAB call after a warm-up, for a
                                                  rocprofv3 --kernel-trace --stats run of its own
  python tests/dev_krylov.py --kernel-stats CSV   each BiCGSTAB kernel's time and bytes/s from the stats CSV of that run
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

N, NC = 1000 * 1000, 64
VEC = N * NC * 8
# vectors of [n][64] float64 each kernel reads plus writes (k_cg_dot: the (r^, v) pass; the ||b||^2 pass at the head of
# every call is the same kernel reading one vector, and the stats row averages over both)
KERNEL_VECS = {"k_cg_dot": 2, "k_cg_xr": 6, "k_bs_tr": 2, "k_bs_xr_full": 7, "k_bs_p": 4, "k_bs_finish": 0}


def setup():
    import hifir_amd
    from oracle import ref
    from util import poisson2d

    A = poisson2d(1000)
    R = ref.RefHIF(A.indptr, A.indices, A.data)
    M = hifir_amd.HIF.from_levels(R.levels(), max_nrhs=64)
    M.set_matrix(A.indptr, A.indices, A.data)
    return A, M


def timed(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure(out_dir):
    import torch

    A, M = setup()
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()
    res = {"workload": "poisson2d(1000), default parameters, 64 columns, torch-device entries", "n": N, "nrhs": NC}

    def mem_first(fn):
        torch.cuda.synchronize()
        f0 = torch.cuda.mem_get_info()[0]
        out = fn()
        torch.cuda.synchronize()
        return f0 - torch.cuda.mem_get_info()[0], out

    taken, _ = mem_first(lambda: M.bicgstab(B, rtol=1e-300, maxit=2))
    res["bicgstab_first_call_bytes"] = int(taken)
    t20, _ = timed(lambda: M.bicgstab(B, rtol=1e-300, maxit=20))
    t40, (_, f40, i40) = timed(lambda: M.bicgstab(B, rtol=1e-300, maxit=40))
    res["bicgstab_ms_per_step"] = (t40 - t20) / 20
    res["bicgstab_t20_t40_ms"] = [t20, t40]
    res["bicgstab_maxit40_flags"] = sorted(set(f40.tolist()))
    ms, (X, fl, it) = timed(lambda: M.bicgstab(B, rtol=1e-8, maxit=1000))
    Xh, Bh = X.cpu().numpy(), B.cpu().numpy()
    rr = np.linalg.norm(A @ Xh - Bh, axis=0) / np.linalg.norm(Bh, axis=0)
    res["bicgstab_to_1e-8"] = {"ms": ms, "flags": sorted(set(fl.tolist())), "steps_min_mean_max":
                               [int(it.min()), float(it.mean()), int(it.max())], "true_relres_max": float(rr.max())}
    del X
    taken, _ = mem_first(lambda: M.gmres(B, restart=30, rtol=1e-300, maxit=2))
    res["gmres30_first_call_bytes"] = int(taken)
    t1, _ = timed(lambda: M.gmres(B, restart=30, rtol=1e-300, maxit=1))
    t30, _ = timed(lambda: M.gmres(B, restart=30, rtol=1e-300, maxit=30))
    res["gmres30_ms_per_inner_step"] = (t30 - t1) / 29
    ms, (X, fl, it) = timed(lambda: M.gmres(B, restart=30, rtol=1e-8, maxit=1000))
    Xh = X.cpu().numpy()
    rr = np.linalg.norm(A @ Xh - Bh, axis=0) / np.linalg.norm(Bh, axis=0)
    res["gmres30_to_1e-8"] = {"ms": ms, "flags": sorted(set(fl.tolist())), "iters_min_mean_max":
                              [int(it.min()), float(it.mean()), int(it.max())], "true_relres_max": float(rr.max())}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "krylov.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def trace(steps):
    import torch

    A, M = setup()
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()
    M.bicgstab(B, rtol=1e-300, maxit=2)  # warm-up: buffers and the apply's graph
    torch.cuda.synchronize()
    _, fl, it = M.bicgstab(B, rtol=1e-300, maxit=steps)
    torch.cuda.synchronize()
    print("trace", steps, "steps:", sorted(set(it.tolist())))


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
    ap.add_argument("--trace-steps", type=int)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats)
    elif a.trace_steps:
        trace(a.trace_steps)
    else:
        measure(a.out or ".")
