"""Development measurement: the basis null-space filter on the 1000^2 pure-Neumann Laplacian (1M rows)
factorized with is_symm by the compiled reference, 64 columns, device-pointer (torch) entries.

  python tests/dev_nsp.py [--out DIR]         PCG ms per step with the basis filter (projected) and without any filter,
                                              iterations to 1e-8 -> DIR/nsp_pcg.json (DIR: .)
  python tests/dev_nsp.py --trace             after a warm-up: the filter alone on a 1M x 64 block for k = 1, 4, 16, the
                                              constant-mode filter on the same block and a 6-step BiCGSTAB call, for a
                                              rocprofv3 --kernel-trace --stats run of its own
  python tests/dev_nsp.py --kernel-stats CSV  each kernel's time and bytes/s from the kernel-trace CSV of that run (bytes
                                              from the shapes: X is n x 64 x 8 B, Q is n x k x 8 B); with --pcg-json FILE
                                              and --profile OUT both results go to OUT (profiles/nsp_filter.json), stamped
                                              with the library's checksum and the git head
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
KS = (1, 4, 16)


def neumann2d(nx):
    T = sp.diags([-1.0, 2.0, -1.0], [-1, 0, 1], shape=(nx, nx), format="lil")
    T[0, 0] = 1.0
    T[nx - 1, nx - 1] = 1.0
    T = T.tocsr()
    I = sp.identity(nx, format="csr")
    A = (sp.kron(I, T) + sp.kron(T, I)).tocsr()
    A.sort_indices()
    return A


def setup():
    import hifir_amd
    from oracle import ref

    A = neumann2d(NX)
    R = ref.RefHIF(A.indptr, A.indices, A.data, ref.make_params(is_symm=1))
    M = hifir_amd.HIF.from_levels(R.levels(), max_nrhs=NC)
    M.set_matrix(A.indptr, A.indices, A.data)
    return A, M


def basis(k):
    """the constants first (the null space), then random vectors to make up k"""
    V = np.random.default_rng(3).uniform(-1, 1, size=(N, k))
    V[:, 0] = 1.0
    return V


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
    assert M.is_hermitian()
    Bh = A @ np.random.default_rng(7).uniform(-1, 1, size=(N, NC))  # consistent: the unfiltered run converges too
    B = torch.from_numpy(Bh).cuda()
    res = {"workload": "neumann2d(1000), is_symm, 64 consistent columns, torch-device entries", "n": N, "nrhs": NC}
    for label, V in (("unfiltered", None), ("basis_k1", np.ones(N))):
        M.set_nsp_basis(V)
        M.pcg(B, rtol=1e-300, maxit=2)  # warm-up: buffers and the apply's graph
        t10, (_, f10, i10) = timed(lambda: M.pcg(B, rtol=1e-300, maxit=10))
        t30, (_, f30, i30) = timed(lambda: M.pcg(B, rtol=1e-300, maxit=30))
        ms, (X, fl, it) = timed(lambda: M.pcg(B, rtol=1e-8, maxit=1000))
        Xh = X.cpu().numpy()
        rr = np.linalg.norm(A @ Xh - Bh, axis=0) / np.linalg.norm(Bh, axis=0)
        res[label] = {"pcg_ms_per_step": (t30 - t10) / 20, "t10_t30_ms": [t10, t30],
                      "maxit30_flags": sorted(set(f30.tolist())), "maxit30_iters": sorted(set(i30.tolist())),
                      "to_1e-8": {"ms": ms, "flags": sorted(set(fl.tolist())), "iters_min_mean_max":
                                  [int(it.min()), float(it.mean()), int(it.max())], "true_relres_max": float(rr.max()),
                                  "mean_over_norm_max": float((np.abs(Xh.sum(axis=0)) / np.sqrt(N) / np.linalg.norm(Xh, axis=0)).max())}}
        del X
    res["nsp_basis_bytes"] = M.stats_ext()["nsp_basis_bytes"]
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "nsp_pcg.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


def trace(reps=5):
    import torch

    A, M = setup()
    X = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()
    for k in KS:
        M.set_nsp_basis(basis(k))
        for _ in range(reps + 1):  # (the first call of every size is the warm-up; the stats average all of them)
            M.nsp_filter(X)
        M.sync()
    M.set_nsp_const(0, -1)
    for _ in range(reps + 1):
        M.nsp_filter(X)
    M.sync()
    M.set_nsp_const(1, 0)
    B = torch.from_numpy(np.random.default_rng(8).uniform(-1, 1, size=(N, NC))).cuda()
    M.bicgstab(B, rtol=1e-300, maxit=2)
    _, fl, it = M.bicgstab(B, rtol=1e-300, maxit=6)
    torch.cuda.synchronize()
    print("trace done; bicgstab steps:", sorted(set(it.tolist())))


def kernel_stats(path):
    """From the per-dispatch kernel trace (the *_kernel_trace.csv of the --trace run): the first dispatch of every
    (kernel, grid) pair is the warm-up and is left out; k_nsp_finish is told apart by its grid (k workgroups)."""
    groups = {}
    for r in csv.DictReader(open(path)):
        name = (r.get("Kernel_Name") or r.get("Name") or "").replace(" ", "")
        m = re.search(r"(k_nsp_coef|k_nsp_sub|k_nsp_finish|k_colsum_partial|k_sub_colmean|k_cg_xr|k_cg_dot|k_bs_finish)<([^>]*)>", name)
        if not m or not m.group(2).startswith("double"):
            continue
        key = m.group(1) + "<" + m.group(2) + ">"
        if m.group(1) == "k_nsp_finish":
            key += " grid %d" % (int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]))
        groups.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    out = {}
    for key, v in sorted(groups.items()):
        d = [dur for _, dur in sorted(v)][1:] or [v[0][1]]
        m = re.match(r"k_nsp_(coef|sub)<double,(\d+)>", key)
        if m:
            nbytes = (1 if m.group(1) == "coef" else 2) * VEC + N * int(m.group(2)) * 8
        else:
            nbytes = {"k_colsum_partial": 1, "k_sub_colmean": 2, "k_cg_xr": 6, "k_cg_dot": 2}.get(key.split("<")[0], 0) * VEC
        us = float(np.mean(d)) / 1e3
        out[key] = {"calls": len(d), "avg_us": us, "min_us": min(d) / 1e3, "bytes": nbytes,
                    "GB_per_s": (nbytes / us / 1e3) if nbytes else None}
    for k in KS:
        parts = [out.get(f"k_nsp_coef<double,{k}>"), out.get(f"k_nsp_finish<double> grid {k}"), out.get(f"k_nsp_sub<double,{k}>")]
        if all(parts):
            us = sum(p["avg_us"] for p in parts)
            nbytes = parts[0]["bytes"] + parts[2]["bytes"]
            out[f"basis_filter_k{k}"] = {"us_per_tile": us, "bytes": nbytes, "GB_per_s": nbytes / us / 1e3}
    if "k_colsum_partial<double>" in out and "k_sub_colmean<double>" in out:
        us = out["k_colsum_partial<double>"]["avg_us"] + out["k_sub_colmean<double>"]["avg_us"]
        out["const_filter"] = {"us_per_tile": us, "bytes": 3 * VEC, "GB_per_s": 3 * VEC / us / 1e3}
    print(json.dumps(out, indent=1))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--pcg-json")
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
                    "kernel_stats_note": "rocprofv3 --kernel-trace --stats of `dev_nsp.py --trace` (a run of its own, no counters): "
                                         "six filter calls per k on a 1M x 64 float64 block, the first left out; bytes from shapes",
                    "kernel_stats": ks}
            if a.pcg_json:
                prof["pcg"] = json.load(open(a.pcg_json))
            with open(a.profile, "w") as f:
                json.dump(prof, f, indent=1)
    elif a.trace:
        trace()
    else:
        measure(a.out or ".")
