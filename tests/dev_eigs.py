"""Development measurement: the locked LOBPCG sweeps on section 4.16's workload -- the 1000^2 Poisson matrix
factorized with make_params(is_symm=1) by the compiled reference, standard and with B = mass2d(1000), nev = 40, k = 16,
guard = 4, tol 1e-8, generated start, device-pointer (torch) entry, one handle, one process.  Not part of the suite.

  python tests/dev_eigs.py [--out DIR] [--hier FILE]
        sweeps, steps and ms to tolerance of eigsh, standard and generalized; the eigenvalues against the closed forms; ms per
        step of the constrained tile at m = 0, 12, 24, 36 locked vectors (REPEATS repeats each) and of lobpcg IN THE SAME
        PROCESS -> DIR/eigs.json.  --hier: as dev_lobpcg_gen.py
  python tests/dev_eigs.py --parent-lib SO [--out DIR] [--hier FILE]
        ms per step of lobpcg with ANOTHER build of the library (the parent commit's); with --out merged into DIR/eigs.json
        with the verdict: this build's m = 0 step does not exceed the parent's median by more than the parent's own spread
  python tests/dev_eigs.py --dump-bits FILE [--parent-lib SO]
        every case of lobpcg_util.CASES / lobpcg_gen_util.GEN_CASES through lobpcg / lobpcg_gen, given and generated start:
        per call the sha256 and the byte count of lambda, X, res, flags, info3 -> FILE
  python tests/dev_eigs.py --compare-bits FILE_A FILE_B [--out DIR]
        the two dumps call by call; with --out merged into DIR/eigs.json
  python tests/dev_eigs.py --trace-project M
        ten projector calls (kw = 16) at M locked vectors on a 10^6-row handle, for a rocprofv3 --kernel-trace --stats run of
        its own
  python tests/dev_eigs.py --kernel-stats FILE --m M [--out DIR]
        the two new kernels' time per launch from the stats CSV or the results database (.db) of that run next to the time
        their bytes need at 8 TB/s (Y or BY plus W read, W written: M + 32 columns of 8 B)
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dev_lobpcg_gen import LO, HI, N, NX, REPEATS, pencil_eigenvalues, per_step, setup  # noqa: E402

NEV, K, GUARD, TOL, SEED = 40, 16, 4, 1e-8, 3
WANT = K - GUARD
MS = (0, 12, 24, 36)
COL = N * 8
NEW_SYMBOLS = ("hifamd_eig_project", "hifamd_eig_project_dev", "hifamd_eigs", "hifamd_eigs_dev", "hifamd_eigs_sweeps")


def poisson_eigenvalues(count):
    """the smallest eigenvalues of poisson2d(NX): c_i + c_j, c_i = 2 - 2 cos(i pi / (NX + 1))"""
    c = 2.0 - 2.0 * np.cos(np.arange(1, 60) * np.pi / (NX + 1))
    return np.sort((c[:, None] + c[None, :]).ravel())[:count]


def use_library(path):
    """point the package at another build of the library; the signatures of entry points it lacks are dropped"""
    import ctypes

    import torch  # noqa: F401  (before the library, as in dev_lobpcg_gen.parent)

    os.environ["HIFIR_AMD_LIB"] = os.path.abspath(path)
    from hifir_amd import _lib

    _lib.LIB_PATH = os.path.abspath(path)
    other = ctypes.CDLL(_lib.LIB_PATH)
    for name in list(_lib.SIGNATURES):
        if not hasattr(other, name):
            _lib.SIGNATURES.pop(name)
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def measure(out_dir, hier):
    import torch
    from dev_blockcg import stamp, timed
    from idrs_util import generated_P

    os.makedirs(out_dir, exist_ok=True)
    A, B, M = setup(hier)
    anorm = float(abs(A).sum(axis=1).max())
    res = {"stamp": stamp(), "workload": "poisson2d(1000), make_params(is_symm=1), standard and B = mass2d(1000), nev 40, k 16, "
           "guard 4, tol 1e-8, generated start, torch-device entry", "n": N, "repeats": REPEATS, "lo_hi": [LO, HI]}
    X0 = torch.empty((N, K), dtype=torch.float64, device="cuda")
    X0.copy_(torch.from_numpy(generated_P(N, K, SEED, False)))
    for gen, key, exact in ((False, "standard", poisson_eigenvalues(NEV)), (True, "generalized", pencil_eigenvalues(NEV))):
        M.eigsh(WANT, k=K, guard=GUARD, gen=gen, X0=X0, tol=1e-300, maxit=2)  # warm-up: buffers, the apply's graph
        ms, (lam, X, r, fl, info) = timed(lambda: M.eigsh(NEV, k=K, guard=GUARD, gen=gen, X0=X0, tol=TOL, maxit=500))
        sweeps = list(M.last_eigsh_sweeps)
        out = {"ms_to_tol": ms, "sweeps": sweeps, "steps": int(info[0]), "info4": info.tolist(), "flags": fl.tolist(),
               "lam": lam.tolist(), "res": r.tolist(),
               "eigenvalue_error_over_anorm": float(np.abs(lam - exact).max() / anorm),
               "ms_per_step_overall": ms / max(int(info[0]), 1)}
        step = {}
        for m in MS:
            Y = X[:, :m].contiguous() if m else None
            reps = per_step(lambda mi: M.eigsh(WANT, k=K, guard=GUARD, gen=gen, Y=Y, X0=X0, tol=1e-300, maxit=mi))
            step[str(m)] = {"ms_per_step": float(np.median(reps)), "repeats": reps}
        out["step_at_m"] = step
        entry = M.lobpcg_gen if gen else M.lobpcg
        reps = per_step(lambda mi: entry(X0=X0, nev=WANT, tol=1e-300, maxit=mi))
        out["lobpcg_ms_per_step"] = float(np.median(reps))
        out["lobpcg_ms_per_step_repeats"] = reps
        res[key] = out
        print(key, json.dumps({k: v for k, v in out.items() if k not in ("lam", "res")}), flush=True)
    with open(os.path.join(out_dir, "eigs.json"), "w") as f:
        json.dump(res, f, indent=1)
    M.close()


def parent(lib_path, out_dir, hier):
    sha = use_library(lib_path)
    import torch
    from idrs_util import generated_P

    A, B, M = setup(hier, mass=False)
    X0 = torch.empty((N, K), dtype=torch.float64, device="cuda")
    X0.copy_(torch.from_numpy(generated_P(N, K, SEED, False)))
    M.lobpcg(X0=X0, nev=WANT, tol=1e-300, maxit=2)
    std = per_step(lambda m: M.lobpcg(X0=X0, nev=WANT, tol=1e-300, maxit=m))
    out = {"parent_lib_sha256": sha, "parent_lobpcg_ms_per_step": float(np.median(std)),
           "parent_lobpcg_ms_per_step_repeats": std, "parent_spread_ms": float(max(std) - min(std))}
    M.close()
    if out_dir:
        p = os.path.join(out_dir, "eigs.json")
        res = json.load(open(p)) if os.path.exists(p) else {}
        res.update(out)
        if "standard" in res:
            mine = res["standard"]["step_at_m"]["0"]["ms_per_step"]
            res["m0_step_within_parent_spread"] = bool(mine <= out["parent_lobpcg_ms_per_step"] + out["parent_spread_ms"])
        with open(p, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(out, indent=1))


def dump_bits(path, lib_path):
    sha = use_library(lib_path) if lib_path else None
    import hifir_amd
    import lobpcg_gen_util as G
    import lobpcg_util as U

    out, handles = {"lib_sha256": sha, "calls": {}}, {}

    def handle(Cs, B):
        key = (Cs.name, B is not None)
        if key not in handles:
            M = hifir_amd.HIF.from_levels(Cs.levels, max_nrhs=64)
            M.set_matrix(Cs.A.indptr, Cs.A.indices, Cs.A.data)
            if B is not None:
                M.set_mass_matrix(B.indptr, B.indices, B.data)
            handles[key] = M
        return handles[key]

    def record(name, call):
        try:
            lam, X, res, fl, steps = call()
        except hifir_amd.HifAmdError as e:
            out["calls"][name] = {"refused": e.code}
            return
        raw = b"".join(np.ascontiguousarray(a).tobytes() for a in (lam, X, res, fl)) + int(steps).to_bytes(4, "little")
        out["calls"][name] = {"sha256": hashlib.sha256(raw).hexdigest(), "bytes": len(raw)}

    for row in U.CASES:
        Cs, solve, X0, k, nev, tol, Q = U.inputs(row[0])
        if Q is not None:
            continue
        M = handle(Cs, None)
        record("lobpcg/" + row[0] + "/given", lambda: M.lobpcg(X0=X0, nev=nev, tol=tol, maxit=U.MAXIT))
        record("lobpcg/" + row[0] + "/generated", lambda: M.lobpcg(k=k, nev=nev, seed=11, tol=tol, maxit=U.MAXIT))
    for row in G.GEN_CASES:
        Cs, solve, B, X0, k, nev, tol = G.inputs(row[0])
        M = handle(Cs, B)
        record("lobpcg_gen/" + row[0] + "/given", lambda: M.lobpcg_gen(X0=X0, nev=nev, tol=tol, maxit=U.MAXIT))
        record("lobpcg_gen/" + row[0] + "/generated", lambda: M.lobpcg_gen(k=k, nev=nev, seed=11, tol=tol, maxit=U.MAXIT))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(len(out["calls"]), "calls,", sum(c.get("bytes", 0) for c in out["calls"].values()), "bytes ->", path)


def compare_bits(a, b, out_dir):
    A, B = json.load(open(a)), json.load(open(b))
    names = sorted(set(A["calls"]) | set(B["calls"]))
    differ = [n for n in names if A["calls"].get(n) != B["calls"].get(n)]
    out = {"bit_check": {"calls": len(names), "ran": sum(1 for n in names if "sha256" in A["calls"].get(n, {})),
                         "bytes": sum(c.get("bytes", 0) for c in A["calls"].values()), "differ": differ,
                         "libs": [A["lib_sha256"], B["lib_sha256"]]}}
    print(json.dumps(out, indent=1))
    if out_dir:
        p = os.path.join(out_dir, "eigs.json")
        res = json.load(open(p)) if os.path.exists(p) else {}
        res.update(out)
        with open(p, "w") as f:
            json.dump(res, f, indent=1)
    return 1 if differ else 0


def trace_project(m):
    import torch

    import hifir_amd
    from lockstep_edges_util import diagonal_levels

    M = hifir_amd.HIF.from_levels(diagonal_levels(np.ones(N)), max_nrhs=16)
    g = torch.Generator(device="cuda").manual_seed(5)
    Y = torch.rand((N, m), dtype=torch.float64, device="cuda", generator=g) / np.sqrt(N)
    W = torch.rand((N, 48), dtype=torch.float64, device="cuda", generator=g)[:, 16:32]  # the W block of S: stride 48
    for _ in range(10):
        M.b_project(W, Y)
    torch.cuda.synchronize()
    print("trace projector, m =", m)


def kernel_rows(path):
    """-> (name, calls, average ns) per kernel from the profiler's stats CSV, or from its database (the `kernels` view)"""
    if path.endswith(".db"):
        import sqlite3

        return list(sqlite3.connect(path).execute("select name, count(*), avg(end - start) from kernels group by name"))
    import csv

    return [(r.get("Name") or r.get("KernelName") or "", int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(path))]


def kernel_stats(path, m, out_dir):
    out = {}
    for name, calls, avg_ns in kernel_rows(path):
        for key in ("k_eig_cgram", "k_eig_cproj", "k_eig_csum"):
            if key in name:
                nbytes = (m + 16 + (16 if key == "k_eig_cproj" else 0)) * COL if key != "k_eig_csum" else 0
                out[key] = {"calls": int(calls), "avg_us": avg_ns / 1e3, "bytes": nbytes,
                            "GB_per_s": nbytes / avg_ns if nbytes else None, "us_at_8TB_per_s": nbytes / 8e6 if nbytes else None}
    print(json.dumps({"m": m, "kernels": out}, indent=1))
    if out_dir:
        p = os.path.join(out_dir, "eigs.json")
        res = json.load(open(p)) if os.path.exists(p) else {}
        res.setdefault("kernel_stats", {})[str(m)] = out
        res["kernel_stats_note"] = ("rocprofv3 --kernel-trace --stats of `dev_eigs.py --trace-project M`, one run per M, no counters; "
                                    "bytes: k_eig_cgram reads BY and W (M + 16 columns), k_eig_cproj reads Y and W and writes W "
                                    "(M + 32 columns), n = 10^6 rows of 8 B")
        with open(p, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--hier")
    ap.add_argument("--parent-lib")
    ap.add_argument("--dump-bits")
    ap.add_argument("--compare-bits", nargs=2)
    ap.add_argument("--trace-project", type=int)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--m", type=int, default=0)
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.m, a.out)
    elif a.compare_bits:
        sys.exit(compare_bits(a.compare_bits[0], a.compare_bits[1], a.out))
    elif a.dump_bits:
        dump_bits(a.dump_bits, a.parent_lib)
    elif a.trace_project:
        trace_project(a.trace_project)
    elif a.parent_lib:
        parent(a.parent_lib, a.out, a.hier)
    else:
        measure(a.out or ".", a.hier)
