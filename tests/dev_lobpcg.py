"""Development measurement: LOBPCG on section 4.7's own workload -- the 1000^2 Poisson matrix factorized with
make_params(is_symm=1) by the compiled reference, k = 16 candidates, nev = 10, tol 1e-8, generated start, device-pointer
(torch) entry, one handle, one process.

  python tests/dev_lobpcg.py [--out DIR]           steps, ms per step, ms to tolerance, memory taken by the first call, the
                                                   eigenvalues against the 2D Poisson formula and the true residuals
                                                   -> DIR/lobpcg.json (stamped with the head and the library)
  python tests/dev_lobpcg.py --trace-steps K       one K-step call after a warm-up, for a rocprofv3 --kernel-trace --stats run
                                                   of its own
  python tests/dev_lobpcg.py --kernel-stats CSV [--out DIR]   each new kernel's time and bytes/s from the stats CSV of that run
                                                   (bytes from the shapes: n = 10^6 rows, 16 / 48 columns, 8 B) next to the
                                                   time those bytes need at 8 TB/s; with --out merged into DIR/lobpcg.json
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

from dev_blockcg import N, NX, setup, stamp, timed  # noqa: E402

K, NEV, TOL, SEED = 16, 10, 1e-8, 3
COL = N * 8  # bytes of one float64 column


def poisson_eigenvalues(count):
    """the smallest eigenvalues of poisson2d(NX): 4 - 2 cos(i pi / (NX + 1)) - 2 cos(j pi / (NX + 1))"""
    c = 2.0 - 2.0 * np.cos(np.arange(1, 40) * np.pi / (NX + 1))
    return np.sort((c[:, None] + c[None, :]).ravel())[:count]


def measure(out_dir):
    import torch

    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "lobpcg.json")
    A, M = setup()
    anorm = float(abs(A).sum(axis=1).max())
    res = {"stamp": stamp(), "workload": "poisson2d(1000), make_params(is_symm=1), k 16, nev 10, tol 1e-8, generated start, "
           "torch-device entry", "n": N, "k": K, "nev": NEV}
    X0 = torch.empty((N, K), dtype=torch.float64, device="cuda")
    from idrs_util import generated_P

    X0.copy_(torch.from_numpy(generated_P(N, K, SEED, False)))
    torch.cuda.synchronize()
    f0 = torch.cuda.mem_get_info()[0]
    M.lobpcg(X0=X0, nev=NEV, tol=1e-300, maxit=2)
    torch.cuda.synchronize()
    res["first_call_bytes"] = int(f0 - torch.cuda.mem_get_info()[0])
    lo, hi = 3, 6
    t_lo, _ = timed(lambda: M.lobpcg(X0=X0, nev=NEV, tol=1e-300, maxit=lo))
    t_hi, _ = timed(lambda: M.lobpcg(X0=X0, nev=NEV, tol=1e-300, maxit=hi))
    ms, (lam, X, r, fl, steps) = timed(lambda: M.lobpcg(X0=X0, nev=NEV, tol=TOL, maxit=500))
    Xh = X.cpu().numpy()
    true = np.linalg.norm(A @ Xh - Xh * lam[None, :], axis=0) / anorm
    res.update(ms_per_step=(t_hi - t_lo) / (hi - lo), t_lo_hi_ms=[t_lo, t_hi], lo_hi=[lo, hi], ms_to_tol=ms, steps=steps,
               flags=fl.tolist(), info3=M.last_lobpcg_info.tolist(), lam=lam.tolist(), res=r.tolist(), true_res=true.tolist(),
               eigenvalue_error_over_anorm=float(np.abs(lam[:NEV] - poisson_eigenvalues(NEV)).max() / anorm),
               orthonormality=float(np.linalg.norm(Xh.T @ Xh - np.eye(K))))
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    M.close()
    print(json.dumps(res, indent=1))


def trace(steps):
    import torch

    A, M = setup()
    M.lobpcg(k=K, nev=NEV, seed=SEED, tol=1e-300, maxit=2)  # warm-up: buffers and the apply's graph
    torch.cuda.synchronize()
    out = M.lobpcg(k=K, nev=NEV, seed=SEED, tol=1e-300, maxit=steps)
    torch.cuda.synchronize()
    print("trace LOBPCG", steps, "steps:", out[4], M.last_lobpcg_info.tolist())


def kernel_key(name):
    """a profiler's kernel name -> its key in SHAPES: the base name, and for the kernels that are instantiated per problem
    (k_lob_gram<T, GEN>, k_lob_update<T, NB>, k_lob_resid<T, GEN>) their last template argument: k_lob_gram<true>"""
    m = re.search(r"(k_lob_\w+)(?:<([^>]*)>)?", name)
    if not m:
        return None
    args = [a.strip() for a in (m.group(2) or "").split(",")]
    return "%s<%s>" % (m.group(1), args[-1]) if len(args) > 1 else m.group(1)


# float64 columns of n rows that a kernel reads plus writes per launch at k = 16
SHAPES = {
    "k_lob_gram<false>": 96,   # S and AS read, 48 columns each
    "k_lob_update<2>": 160,    # S and AS read (96), X, P, AX, AP written (64)
    "k_lob_resid<false>": 48,  # X, AX read, R written
    "k_lob_lock": 0,           # writes converged columns only
    "k_lob_small": 0,
}


def kernel_stats(path, out_dir, shapes=SHAPES, json_name="lobpcg.json", script="dev_lobpcg.py"):
    out = {}
    for r in csv.DictReader(open(path)):
        key = kernel_key(r.get("Name") or r.get("KernelName") or "")
        if key not in shapes:
            continue
        nbytes = shapes[key] * COL
        avg_ns = float(r["AverageNs"])
        out[key] = {"calls": int(r["Calls"]), "avg_us": avg_ns / 1e3, "bytes": nbytes,
                           "GB_per_s": nbytes / avg_ns if nbytes else None, "us_at_8TB_per_s": nbytes / 8e6 if nbytes else None}
    print(json.dumps(out, indent=1))
    if out_dir:
        p = os.path.join(out_dir, json_name)
        res = json.load(open(p)) if os.path.exists(p) else {}
        res["kernel_stats_note"] = ("rocprofv3 --kernel-trace --stats of `%s --trace-steps` (a run of its own, no "
                                    "counters); bytes from the shapes at k = 16" % script)
        res["kernel_stats"] = out
        with open(p, "w") as f:
            json.dump(res, f, indent=1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace-steps", type=int)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.out)
    elif a.trace_steps:
        trace(a.trace_steps)
    else:
        measure(a.out or ".")
