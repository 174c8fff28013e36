"""Development measurement: generalized LOBPCG on section 4.16's workload -- the 1000^2 Poisson matrix
factorized with make_params(is_symm=1) by the compiled reference, B = mass2d(1000) (lobpcg_gen_util), k = 16 candidates,
nev = 10, tol 1e-8, generated start, device-pointer (torch) entry, one handle, one process.

  python tests/dev_lobpcg_gen.py [--out DIR] [--hier FILE]
        steps and ms to tolerance, ms per step of lobpcg_gen and of lobpcg IN THE SAME PROCESS (REPEATS repeats each), memory
        taken by the first call, the eigenvalues against the pencil's closed form, the true backward errors
        -> DIR/lobpcg_gen.json (stamped with the head and the library).  --hier: the factorized hierarchy is read from FILE
        (hifamd_load) when it exists and written there when not, so that further runs do not factorize again
  python tests/dev_lobpcg_gen.py --parent-lib SO [--out DIR] [--hier FILE]
        ms per step of the standard lobpcg, and of lobpcg_gen where it has it, with ANOTHER build of the library (the parent
        commit's), same repeats; with --out merged into DIR/lobpcg_gen.json next to this build's figures and the verdicts:
        this build's median does not exceed the parent's by more than the spread (max - min) of the parent's own repeats
  python tests/dev_lobpcg_gen.py --trace-steps K [--hier FILE]
        one K-step call after a warm-up, for a rocprofv3 --kernel-trace --stats run of its own
  python tests/dev_lobpcg_gen.py --kernel-stats CSV [--out DIR]
        each new kernel's time and bytes/s from the stats CSV of that run (bytes from the shapes: n = 10^6 rows, 16 / 48
        columns, 8 B) next to the time those bytes need at 8 TB/s; with --out merged into DIR/lobpcg_gen.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, NEV, TOL, SEED = 16, 10, 1e-8, 3
NX = 1000
N = NX * NX
COL = N * 8  # bytes of one float64 column
REPEATS = 5
LO, HI = 3, 6
NEW_SYMBOLS = ("hifamd_set_mass_matrix", "hifamd_lobpcg_gen", "hifamd_lobpcg_gen_dev")


def pencil_eigenvalues(count):
    """the smallest eigenvalues of the pencil (poisson2d(NX), mass2d(NX)): A = kron(T1, I) + kron(I, T1) and B = kron(T, T)
    share the sine modes as eigenvectors; with c_i = 2 - 2 cos(i pi / (NX + 1)) and m_i = (4 + 2 cos(i pi / (NX + 1))) / 6,
    lambda_ij = (c_i + c_j) / (m_i m_j)"""
    th = np.arange(1, 40) * np.pi / (NX + 1)
    c, m = 2.0 - 2.0 * np.cos(th), (4.0 + 2.0 * np.cos(th)) / 6.0
    return np.sort(((c[:, None] + c[None, :]) / (m[:, None] * m[None, :])).ravel())[:count]


def setup(hier, mass=True):
    import hifir_amd
    from dev_blockcg import setup as factorize
    from lobpcg_gen_util import mass2d
    from util import poisson2d

    if hier and os.path.exists(hier):
        A = poisson2d(NX)
        t0 = time.perf_counter()
        M = hifir_amd.HIF.load(hier, max_nrhs=64)
        M.set_matrix(A.indptr, A.indices, A.data)
        print("loaded %s in %.1f s" % (hier, time.perf_counter() - t0), flush=True)
        assert M.is_hermitian()
    else:
        A, M = factorize()
        if hier:
            M.save(hier)
    B = mass2d(NX)
    if mass:
        M.set_mass_matrix(B.indptr, B.indices, B.data)
    return A, B, M


def per_step(call):
    """REPEATS figures of (t(HI steps) - t(LO steps)) / (HI - LO) in ms"""
    from dev_blockcg import timed

    out = []
    for _ in range(REPEATS):
        t_lo, _ = timed(lambda: call(LO))
        t_hi, _ = timed(lambda: call(HI))
        out.append((t_hi - t_lo) / (HI - LO))
    return out


def start_block():
    import torch
    from idrs_util import generated_P

    X0 = torch.empty((N, K), dtype=torch.float64, device="cuda")
    X0.copy_(torch.from_numpy(generated_P(N, K, SEED, False)))
    torch.cuda.synchronize()
    return X0


def measure(out_dir, hier):
    import torch
    from dev_blockcg import stamp, timed

    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "lobpcg_gen.json")
    A, B, M = setup(hier)
    anorm, bnorm = float(abs(A).sum(axis=1).max()), float(abs(B).sum(axis=1).max())
    res = {"stamp": stamp(), "workload": "poisson2d(1000), make_params(is_symm=1), B = mass2d(1000), k 16, nev 10, tol 1e-8, "
           "generated start, torch-device entry", "n": N, "k": K, "nev": NEV, "repeats": REPEATS, "lo_hi": [LO, HI]}
    X0 = start_block()
    f0 = torch.cuda.mem_get_info()[0]
    M.lobpcg_gen(X0=X0, nev=NEV, tol=1e-300, maxit=2)
    torch.cuda.synchronize()
    res["first_call_bytes"] = int(f0 - torch.cuda.mem_get_info()[0])
    M.lobpcg(X0=X0, nev=NEV, tol=1e-300, maxit=2)
    gen = per_step(lambda m: M.lobpcg_gen(X0=X0, nev=NEV, tol=1e-300, maxit=m))
    std = per_step(lambda m: M.lobpcg(X0=X0, nev=NEV, tol=1e-300, maxit=m))
    ms, (lam, X, r, fl, steps) = timed(lambda: M.lobpcg_gen(X0=X0, nev=NEV, tol=TOL, maxit=500))
    info = M.last_lobpcg_info.tolist()
    ms_std, out_std = timed(lambda: M.lobpcg(X0=X0, nev=NEV, tol=TOL, maxit=500))
    Xh = X.cpu().numpy()
    BX = B @ Xh
    true = np.linalg.norm(A @ Xh - BX * lam[None, :], axis=0) / ((anorm + np.abs(lam) * bnorm) * np.linalg.norm(Xh, axis=0))
    res.update(ms_per_step=float(np.median(gen)), ms_per_step_repeats=gen, lobpcg_ms_per_step=float(np.median(std)),
               lobpcg_ms_per_step_repeats=std, ms_to_tol=ms, steps=steps, flags=fl.tolist(), info3=info,
               lobpcg_ms_to_tol=ms_std, lobpcg_steps=out_std[4], lam=lam.tolist(), res=r.tolist(), true_res=true.tolist(),
               eigenvalue_error_over_anorm=float(np.abs(lam[:NEV] - pencil_eigenvalues(NEV)).max() / anorm),
               b_orthonormality=float(np.linalg.norm(Xh.T @ BX - np.eye(K))))
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    M.close()
    print(json.dumps(res, indent=1))


def parent(lib_path, out_dir, hier):
    """both drivers' steps with another build of the library (the parent commit's); the signatures of entry points that build
    lacks are dropped, and the generalized step is measured only where it has them"""
    import ctypes
    import hashlib

    import torch  # noqa: F401  (before the library, as in measure(): torch found no GPU when its runtime came second)

    os.environ["HIFIR_AMD_LIB"] = os.path.abspath(lib_path)
    from hifir_amd import _lib

    _lib.LIB_PATH = os.path.abspath(lib_path)
    other = ctypes.CDLL(_lib.LIB_PATH)
    has_gen = all(hasattr(other, name) for name in NEW_SYMBOLS)
    for name in NEW_SYMBOLS:
        if not has_gen:
            _lib.SIGNATURES.pop(name, None)
    A, B, M = setup(hier, mass=has_gen)
    X0 = start_block()
    M.lobpcg(X0=X0, nev=NEV, tol=1e-300, maxit=2)
    if has_gen:
        M.lobpcg_gen(X0=X0, nev=NEV, tol=1e-300, maxit=2)
    gen = per_step(lambda m: M.lobpcg_gen(X0=X0, nev=NEV, tol=1e-300, maxit=m)) if has_gen else None
    std = per_step(lambda m: M.lobpcg(X0=X0, nev=NEV, tol=1e-300, maxit=m))
    out = {"parent_lib_sha256": hashlib.sha256(open(lib_path, "rb").read()).hexdigest(),
           "parent_lobpcg_ms_per_step": float(np.median(std)), "parent_lobpcg_ms_per_step_repeats": std,
           "parent_spread_ms": float(max(std) - min(std))}
    if has_gen:
        out.update(parent_ms_per_step=float(np.median(gen)), parent_ms_per_step_repeats=gen,
                   parent_gen_spread_ms=float(max(gen) - min(gen)))
    M.close()
    if out_dir:
        p = os.path.join(out_dir, "lobpcg_gen.json")
        res = json.load(open(p)) if os.path.exists(p) else {}
        res.update(out)
        if "lobpcg_ms_per_step" in res:
            res["standard_step_within_parent_spread"] = bool(
                res["lobpcg_ms_per_step"] <= out["parent_lobpcg_ms_per_step"] + out["parent_spread_ms"])
        if has_gen and "ms_per_step" in res:
            res["generalized_step_within_parent_spread"] = bool(
                res["ms_per_step"] <= out["parent_ms_per_step"] + out["parent_gen_spread_ms"])
        with open(p, "w") as f:
            json.dump(res, f, indent=1)
        out = res
    print(json.dumps({k: v for k, v in out.items() if "ms_per_step" in k or "parent" in k}, indent=1))


def trace(steps, hier):
    import torch

    A, B, M = setup(hier)
    M.lobpcg_gen(k=K, nev=NEV, seed=SEED, tol=1e-300, maxit=2)  # warm-up: buffers and the apply's graph
    torch.cuda.synchronize()
    out = M.lobpcg_gen(k=K, nev=NEV, seed=SEED, tol=1e-300, maxit=steps)
    torch.cuda.synchronize()
    print("trace generalized LOBPCG", steps, "steps:", out[4], M.last_lobpcg_info.tolist())


# float64 columns of n rows that a kernel reads plus writes per launch at k = 16 (keys: dev_lobpcg.kernel_key)
SHAPES = {
    "k_lob_gram<true>": 144,   # S, BS and AS read, 48 columns each
    "k_lob_update<3>": 240,    # S, AS and BS read (144), X, P, AX, AP, BX, BP written (96)
    "k_lob_resid<true>": 64,   # X, AX, BX read, R written
    "k_lob_lock": 0,           # writes converged columns only
    "k_lob_small": 0,
}


def kernel_stats(path, out_dir):
    from dev_lobpcg import kernel_stats as stats

    return stats(path, out_dir, SHAPES, "lobpcg_gen.json", "dev_lobpcg_gen.py")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--hier")
    ap.add_argument("--parent-lib")
    ap.add_argument("--trace-steps", type=int)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats, a.out)
    elif a.parent_lib:
        parent(a.parent_lib, a.out, a.hier)
    elif a.trace_steps:
        trace(a.trace_steps, a.hier)
    else:
        measure(a.out or ".", a.hier)
