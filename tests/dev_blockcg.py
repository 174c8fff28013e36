"""Development measurement: block CG at block 16 and 64 next to PCG on section 4.7's own workload -- the 1000^2
Poisson matrix factorized with make_params(is_symm=1) by the compiled reference, 64 columns, rtol 1e-8, device-pointer (torch)
entries, one handle, one process.

  python tests/dev_blockcg.py [--out DIR]          iterations, ms per step, ms to 1e-8, memory taken by the first call and true
                                                   residuals -> DIR/blockcg_krylov.json (stamped with the head and the library)
  python tests/dev_blockcg.py --trace-steps K [--block S]   one K-step block CG call after a warm-up, for a
                                                   rocprofv3 --kernel-trace --stats run of its own
  python tests/dev_blockcg.py --kernel-stats CSV [--out DIR]   each new kernel's time, bytes/s and flop/s from the stats CSV of
                                                   that run (bytes and flops from the shapes: n = 10^6 rows, 64 columns, 8 B);
                                                   with --out merged into DIR/blockcg_krylov.json
"""
import argparse
import csv
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NC = 1000, 64
N = NX * NX
VEC = N * NC * 8
RTOL = 1e-8


def stamp():
    so = os.path.join(ROOT, "hifir_amd", "libhifir_amd.so")
    out = {"lib_sha256": hashlib.sha256(open(so, "rb").read()).hexdigest() if os.path.exists(so) else None}
    try:
        out["git_head"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        out["csrc_dirty"] = bool(subprocess.check_output(
            ["git", "-C", ROOT, "status", "--porcelain", "--", "hifir_amd/csrc", "include"], text=True, stderr=subprocess.DEVNULL).strip())
    except Exception:
        head = os.path.join(ROOT, ".git_head")
        out["git_head"] = open(head).read().strip() if os.path.exists(head) else None
        out["csrc_dirty"] = None
    return out


def setup():
    import hifir_amd
    from oracle import ref
    from util import poisson2d

    A = poisson2d(NX)
    t0 = time.perf_counter()
    R = ref.RefHIF(A.indptr, A.indices, A.data, ref.make_params(is_symm=1))
    levels = R.levels()
    print("factorized in %.1f s, %d levels" % (time.perf_counter() - t0, len(levels)), flush=True)
    M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
    M.set_matrix(A.indptr, A.indices, A.data)
    assert M.is_hermitian()
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

    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "blockcg_krylov.json")
    A, M = setup()
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()
    Bh = B.cpu().numpy()
    bn = np.linalg.norm(Bh, axis=0)
    res = {"stamp": stamp(), "workload": "poisson2d(1000), make_params(is_symm=1), 64 columns, rtol 1e-8, torch-device entries",
           "n": N, "nrhs": NC}

    def mem_first(fn):
        torch.cuda.synchronize()
        f0 = torch.cuda.mem_get_info()[0]
        out = fn()
        torch.cuda.synchronize()
        return f0 - torch.cuda.mem_get_info()[0], out

    def one(name, run, lo, hi):
        """run(maxit, rtol) -> (X, flags, iters[, ranks]); ms per step from two maxit-capped calls after the warm-up call"""
        taken, _ = mem_first(lambda: run(2, 1e-300))
        t_lo, _ = timed(lambda: run(lo, 1e-300))
        t_hi, out_hi = timed(lambda: run(hi, 1e-300))
        ms, out = timed(lambda: run(1000, RTOL))
        X, fl, it = out[:3]
        rr = np.linalg.norm(A @ X.cpu().numpy() - Bh, axis=0) / bn
        del X
        r = {"first_call_bytes": int(taken), "ms_per_step": (t_hi - t_lo) / (hi - lo), "t_lo_hi_ms": [t_lo, t_hi], "lo_hi": [lo, hi],
             "capped_flags": sorted(set(out_hi[1].tolist())), "ms_to_1e-8": ms, "flags": sorted(set(fl.tolist())),
             "steps_min_mean_max": [int(it.min()), float(it.mean()), int(it.max())], "true_relres_max": float(rr.max())}
        if len(out) > 3:
            r["ranks"] = out[3].tolist()
        res[name] = r
        print(name, json.dumps(r), flush=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)

    # (a capped call stops early where the block converges below 1e-300 -- it cannot; the caps stay under each solver's count)
    one("pcg", lambda maxit, rtol: M.pcg(B, rtol=rtol, maxit=maxit), 3, 6)
    one("bcg64", lambda maxit, rtol: M.bcg(B, block=64, rtol=rtol, maxit=maxit), 2, 4)
    one("bcg16", lambda maxit, rtol: M.bcg(B, block=16, rtol=rtol, maxit=maxit), 2, 4)
    M.close()
    print(json.dumps(res, indent=1))


def trace(steps, block):
    import torch

    A, M = setup()
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()
    M.bcg(B, block=block, rtol=1e-300, maxit=2)  # warm-up: buffers and the apply's graph
    torch.cuda.synchronize()
    _, fl, it, rk = M.bcg(B, block=block, rtol=1e-300, maxit=steps)
    torch.cuda.synchronize()
    print("trace block CG, block", block, steps, "steps:", sorted(set(it.tolist())), rk.tolist())


# [n][64] float64 vectors a kernel reads plus writes, and its flops per row (64 columns, rank 64)
SHAPES = {
    "k_bcg_gram": (2, 2 * 64 * 64),                 # X, Y read; X^H Y
    "k_bcg_xq": (6, 3 * 2 * 64 * 64),               # P, T, X, Q read, X, Q written; P E1, T E2, Q^H Q
    "k_bcg_qp": (5, 3 * 2 * 64 * 64),               # Q, W, P read, Q, P written; Q E1, W E1, P E2
    "k_bcg_norm": (2, 64),
    "k_bcg_sum": (0, 0),
    "k_bcg_small": (0, 0),
    "k_bcg_beta": (0, 0),
}


def kernel_stats(path, out_dir):
    out = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        m = re.search(r"(k_bcg_\w+)", name)
        if not m:
            continue
        nv, fl = SHAPES[m.group(1)]
        avg_ns = float(r["AverageNs"])
        key = re.search(r"(k_bcg_\w+(<[^>]*>)?)", name).group(1)
        out[key] = {"calls": int(r["Calls"]), "avg_us": avg_ns / 1e3, "bytes": nv * VEC, "GB_per_s": (nv * VEC / avg_ns) if nv else None,
                    "Gflop_per_s": (fl * N / avg_ns) if fl else None}
    print(json.dumps(out, indent=1))
    if out_dir:
        p = os.path.join(out_dir, "blockcg_krylov.json")
        res = json.load(open(p)) if os.path.exists(p) else {}
        res["kernel_stats_note"] = ("rocprofv3 --kernel-trace --stats of `dev_blockcg.py --trace-steps` (a run of its own, no counters); "
                                    "bytes and flops from the shapes at rank 64")
        res["kernel_stats"] = out
        with open(p, "w") as f:
            json.dump(res, f, indent=1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace-steps", type=int)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.out)
    elif a.trace_steps:
        trace(a.trace_steps, a.block)
    else:
        measure(a.out or ".")
