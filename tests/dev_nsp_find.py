"""Development measurement: the null-space search on the 1000^2 pure-Neumann Laplacian (1M rows)
factorized with is_symm by the compiled reference (the workload of tests/dev_nsp.py), defaults rtol = 1e-10,
tol = 1e-7, restart 30, maxit 500.

  python tests/dev_nsp_find.py [--out DIR]         wall time of one find_nullspace (second call: buffers and graphs
                                                   warm), of a bare 16-column gmres on the same B = -A X0 with the same
                                                   arguments (the yardstick: that call exists without the search), GMRES
                                                   iterations, the residuals -> DIR/nsp_find_times.json (DIR: .)
  python tests/dev_nsp_find.py --trace             two find_nullspace calls for a rocprofv3 --kernel-trace --stats run
                                                   of its own
  python tests/dev_nsp_find.py --kernel-stats CSV  per-kernel times of the search's own kernels from the kernel-trace
                                                   CSV of that run (bytes from the shapes: V is n x 16 x 8 B, read
                                                   once by the Gram pass -- as X and as Q --, read and written by k_blk_rmul); with
                                                   --times-json FILE and --profile OUT both results go to OUT
                                                   (profiles/nsp_find.json), stamped with the library's checksum and
                                                   the git head
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dev_nsp import N, setup  # noqa: E402  (the same matrix and hierarchy)
from test_nsp_find_host import _probe_numpy  # noqa: E402

K = 16
BLK = N * K * 8


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def measure(out_dir):
    A, M = setup()
    X0 = _probe_numpy(N, 0, False)
    B = -(A @ X0)
    M.find_nullspace(install=False)  # warm-up
    ms_find, (Q, resid, info) = timed(lambda: M.find_nullspace(install=False))
    ms_find_x0, (Q1, _, _) = timed(lambda: M.find_nullspace(install=False, X0=X0))
    M.gmres(B, restart=30, rtol=1e-10, maxit=500)
    ms_gmres, (D, fl, it) = timed(lambda: M.gmres(B, restart=30, rtol=1e-10, maxit=500))
    q = Q[:, 0]
    sigma = 2.0 - 2.0 * np.cos(np.pi / 1000)
    res = {"workload": "neumann2d(1000), is_symm, 16 probe columns, host entries (the gmres yardstick moves B and X over "
                       "PCIe: 2 x 128 MB; the search moves nothing but Q)",
           "n": N, "find_ms": ms_find, "find_explicit_X0_ms": ms_find_x0, "bare_gmres16_ms": ms_gmres,
           "outside_gmres_share_upper_bound": (ms_find - ms_gmres) / ms_find,
           "same_bits_X0_vs_seed": bool(np.array_equal(Q, Q1)),
           "gmres_iters_min_max": [int(it.min()), int(it.max())], "gmres_flags": sorted(set(fl.tolist())),
           "found": int(Q.shape[1]), "info": info, "resid": resid.tolist(),
           "A_q_norm": float(np.linalg.norm(A @ q)), "q_minus_mean_norm": float(np.linalg.norm(q - q.mean())),
           "bound": float(np.linalg.norm(A @ q) / sigma)}
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "nsp_find_times.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def trace():
    A, M = setup()
    for _ in range(2):
        Q, resid, info = M.find_nullspace(install=False)
    print("trace done:", Q.shape, info)


def kernel_stats(path):
    """From the per-dispatch kernel trace: the search's own kernels (k_probe_fill, k_blk_rmul, and k_nsp_coef<16> /
    k_nsp_finish as the Gram reduction); the first dispatch of every kernel is the warm-up and is left out."""
    groups = {}
    total = {}
    for r in csv.DictReader(open(path)):
        name = (r.get("Kernel_Name") or r.get("Name") or "").replace(" ", "")
        dur = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        short = re.sub(r"\(.*", "", re.sub(r"^void", "", name))
        total[short] = total.get(short, 0) + dur
        m = re.search(r"(k_probe_fill|k_blk_rmul|k_nsp_coef|k_nsp_finish|k_colnorm2_partial)<([^>]*)>", name)
        if not m or not m.group(2).startswith("double"):
            continue
        groups.setdefault(m.group(1) + "<" + m.group(2) + ">", []).append((int(r["Start_Timestamp"]), dur))
    out = {}
    for key, v in sorted(groups.items()):
        d = [dur for _, dur in sorted(v)][1:] or [v[0][1]]
        nbytes = {"k_probe_fill": 1, "k_blk_rmul": 2, "k_nsp_coef": 1, "k_colnorm2_partial": 1}.get(key.split("<")[0], 0) * BLK
        us = float(np.mean(d)) / 1e3
        out[key] = {"calls": len(d), "avg_us": us, "min_us": min(d) / 1e3, "bytes": nbytes,
                    "GB_per_s": (nbytes / us / 1e3) if nbytes else None}
    all_us = sum(total.values()) / 1e3
    own_us = sum(v for k, v in total.items() if re.search(r"k_probe_fill|k_blk_rmul|k_nsp_coef|k_nsp_finish|k_colnorm2_partial", k)) / 1e3
    out["device_time_us_all_kernels"] = all_us
    out["device_time_us_search_own_kernels"] = own_us
    out["search_own_share_of_device_time"] = own_us / all_us if all_us else None
    print(json.dumps(out, indent=1))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--times-json")
    ap.add_argument("--profile")
    a = ap.parse_args()
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        if a.profile:
            import hashlib
            import subprocess

            so = os.path.join(ROOT, "hifir_amd", "libhifir_amd.so")
            stamp = {"lib_sha256": hashlib.sha256(open(so, "rb").read()).hexdigest() if os.path.exists(so) else None}
            try:
                stamp["git_head"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
                stamp["csrc_dirty"] = bool(subprocess.check_output(
                    ["git", "-C", ROOT, "status", "--porcelain", "--", "hifir_amd/csrc", "include"], text=True).strip())
            except Exception:
                stamp["git_head"] = stamp["csrc_dirty"] = None
            prof = {"stamp": stamp,
                    "kernel_stats_note": "rocprofv3 --kernel-trace --stats of `dev_nsp_find.py --trace` (a run of its own, no "
                                         "counters): two find_nullspace calls on the 1M-row Neumann Laplacian, the first "
                                         "dispatch of every kernel left out; bytes from shapes (V is 1M x 16 float64)",
                    "kernel_stats": ks}
            if a.times_json:
                prof["times"] = json.load(open(a.times_json))
            with open(a.profile, "w") as f:
                json.dump(prof, f, indent=1)
    elif a.trace:
        trace()
    else:
        measure(a.out or ".")
