"""Development measurement: restarted block GCR next to BiCGSTAB, GMRES(30) and IDR(4) on section 4.13's two
workloads -- the 1000^2 Poisson matrix and the convection-dominated matrix of the same size (dev_idrs.convdiff2d, eps = 2e-4),
both factorized with default parameters by the compiled reference -- 64 columns, rtol 1e-8, device-pointer (torch) entries,
one handle and one process per workload.

  python tests/dev_blockgcr.py [--out DIR] [--only poisson|convdiff]   per solver ms per step, steps and ms to 1e-8, the
                                                   largest true residual, ranks and the memory its first call takes
                                                   -> DIR/blockgcr_krylov.json (stamped with the head and the library)
  python tests/dev_blockgcr.py --trace-steps K [--block S] [--restart M]   one K-step block GCR call after a warm-up, for a
                                                   rocprofv3 --kernel-trace --stats run of its own
  python tests/dev_blockgcr.py --kernel-stats CSV [--out DIR]   each new kernel's time, bytes/s and flop/s from the stats CSV
                                                   of that run (bytes and flops from the shapes: n = 10^6 rows, 64 columns,
                                                   8 B, averaged over the stack depths 0 .. K - 1 of a K-step cycle)
"""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dev_blockcg import stamp  # noqa: E402
from dev_idrs import N, NC, VEC, setup, timed  # noqa: E402

RTOL = 1e-8


def measure_one(which, res, save):
    import torch

    A, M = setup(which)
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()
    Bh = B.cpu().numpy()
    bn = np.linalg.norm(Bh, axis=0)

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
             "capped_flags": sorted(set(out_hi[1].tolist())), "capped_steps": sorted(set(out_hi[2].tolist())), "ms_to_1e-8": ms,
             "flags": sorted(set(fl.tolist())), "steps_min_mean_max": [int(it.min()), float(it.mean()), int(it.max())],
             "true_relres_max": float(rr.max())}
        if len(out) > 3:
            r["ranks"] = out[3].tolist()
        res[which][name] = r
        print(which, name, json.dumps(r), flush=True)
        save()

    # (block GCR's caps are one step and one full cycle: their difference is the steps at the stack depths 1 .. restart - 1)
    one("bgcr64_r10", lambda maxit, rtol: M.bgcr(B, block=64, restart=10, rtol=rtol, maxit=maxit), 1, 10)
    one("bgcr64_r20", lambda maxit, rtol: M.bgcr(B, block=64, restart=20, rtol=rtol, maxit=maxit), 1, 20)
    one("bgcr16_r10", lambda maxit, rtol: M.bgcr(B, block=16, restart=10, rtol=rtol, maxit=maxit), 1, 10)
    one("bicgstab", lambda maxit, rtol: M.bicgstab(B, rtol=rtol, maxit=maxit), 20, 40)
    one("gmres30", lambda maxit, rtol: M.gmres(B, restart=30, rtol=rtol, maxit=maxit), 1, 30)
    one("idrs4", lambda maxit, rtol: M.idrs(B, s=4, rtol=rtol, maxit=maxit), 18, 36)
    M.close()


def measure(out_dir, only):
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "blockgcr_krylov.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    res["stamp"] = stamp()
    res["workloads"] = {"poisson": "poisson2d(1000), default parameters, 64 columns, rtol 1e-8, torch-device entries",
                        "convdiff": "convdiff2d(1000, eps = 2e-4), default parameters, 64 columns, rtol 1e-8, torch-device entries"}

    def save():
        with open(path, "w") as f:
            json.dump(res, f, indent=1)

    for which in ("poisson", "convdiff"):
        if only in (None, which):
            res[which] = {"n": N, "nrhs": NC}
            measure_one(which, res, save)
    print(json.dumps(res, indent=1))


def trace(steps, block, restart):
    import torch

    A, M = setup("poisson")
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()
    M.bgcr(B, block=block, restart=restart, rtol=1e-300, maxit=2)  # warm-up: buffers and the apply's graph
    torch.cuda.synchronize()
    _, fl, it, rk = M.bgcr(B, block=block, restart=restart, rtol=1e-300, maxit=steps)
    torch.cuda.synchronize()
    print("trace block GCR, block", block, "restart", restart, steps, "steps:", sorted(set(it.tolist())), rk.tolist())


def shapes(depth):
    """kernel -> ([n][64] float64 blocks read plus written, flops per row) at rank 64, averaged over the stack depths
    0 .. depth - 1 (k_bgcr_gram runs from depth 1 on: its average is over 1 .. depth - 1)"""
    j = (depth - 1) / 2.0
    jg = depth / 2.0
    return {
        "k_bgcr_gram": (jg + 1, jg * 2 * 64 * 64),             # the stack and W read (W once: the stack index runs fastest)
        "k_bgcr_proj": (2 * j + 4, (2 * j + 1) * 2 * 64 * 64),  # Q_i, P_i, W, Z read, W, Z written; the two updates, W^H W
        "k_bgcr_rmul": (3, 1.5 * 2 * 64 * 64),                  # (two calls on two blocks, one on one: 1.5 blocks a call)
        "k_bgcr_sum": (0, 0),
        "k_bgcr_small": (0, 0),
        "k_bgcr_rho": (0, 0),
    }


def kernel_stats(path, out_dir, depth):
    out = {}
    S = shapes(depth)
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        m = re.search(r"(k_bgcr_\w+)", name)
        if not m:
            continue
        nv, fl = S[m.group(1)]
        avg_ns = float(r["AverageNs"])
        key = re.search(r"(k_bgcr_\w+(<[^>]*>)?)", name).group(1)
        out[key] = {"calls": int(r["Calls"]), "avg_us": avg_ns / 1e3, "min_us": float(r["MinNs"]) / 1e3 if r.get("MinNs") else None,
                    "bytes": nv * VEC, "GB_per_s": (nv * VEC / avg_ns) if nv else None,
                    "Gflop_per_s": (fl * N / avg_ns) if fl else None}
    print(json.dumps(out, indent=1))
    if out_dir:
        p = os.path.join(out_dir, "blockgcr_krylov.json")
        res = json.load(open(p)) if os.path.exists(p) else {}
        res["kernel_stats_note"] = ("rocprofv3 --kernel-trace --stats of `dev_blockgcr.py --trace-steps %d` (a run of its own, no "
                                    "counters); bytes and flops from the shapes at rank 64, averaged over the cycle's depths" % depth)
        res["kernel_stats"] = out
        with open(p, "w") as f:
            json.dump(res, f, indent=1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", choices=["poisson", "convdiff"])
    ap.add_argument("--trace-steps", type=int)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--restart", type=int, default=10)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.out, a.trace_steps or 10)
    elif a.trace_steps:
        trace(a.trace_steps, a.block, a.restart)
    else:
        measure(a.out or ".", a.only)
