"""Development measurement: BiCGSTAB next to GMRES(30) on the bench workload, the 1000^2 Poisson matrix
factorized with default parameters by the compiled reference, 64 columns, device-pointer (torch) entries.

  python tests/dev_krylov.py [--out DIR]          memory, ms per step, steps and time to 1e-8 -> DIR/krylov.json (DIR: .)
  python tests/dev_krylov.py --trace-steps K      one K-step BiCGSTAB call after a warm-up, for a
                                                  rocprofv3 --kernel-trace --stats run of its own
  python tests/dev_krylov.py --kernel-stats CSV   each BiCGSTAB kernel's time and bytes/s from the stats CSV of that run
                                                  (bytes from the shapes: n = 10^6 rows, 64 columns, 8 B)
  python tests/dev_krylov.py --parent-lib SO [--what identity|speed|both] [--parent-first] [--out DIR]
        this build next to ANOTHER build of the library (the parent commit's), both loaded into one process:
        identity: gmres, fgmres, gmres_ir, hifir (unbounded and bounded), find_nullspace, lobpcg, lobpcg_gen, bcg, bgcr and pcg
                  on the small hierarchies of the GPU tests, real and complex, widths 1, 17, 64, 65, restarts 1, 5, 30, a zero
                  and a NaN column in every batch, host and device-pointer forms; every output array byte for byte
        speed:    GMRES(30) ms per inner step, GMRES-IR with the defaults and LOBPCG ms per step on the 1M-row workload, the
                  median of five repeats against the min .. max of the parent's five; --parent-first: the parent's handle is
                  made first and goes first in every pair (-> "speed_parent_first")
        -> DIR/readback_refactor.json (stamped with the head, this library and the parent's sha256); exit status 1 when a byte
        differs
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


# ---- this build next to another build of the library (the parent commit's), both loaded into ONE process -----------------------
WIDTHS, RESTARTS = (1, 17, 64, 65), (1, 5, 30)
ZERO_COL, NAN_COL = 3, 5  # of every batch wider than NAN_COL
REPEATS = 5


def load_library(path):
    """another build of the library, with the signatures of hifir_amd._lib"""
    import ctypes

    from hifir_amd import _lib

    _lib.lib()  # (this build first: it brings torch's HIP runtime in ahead of both)
    L = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


class serving:
    """with serving(L): every hifir_amd call goes to the library L"""

    def __init__(self, L):
        self.L = L

    def __enter__(self):
        from hifir_amd import _lib

        self.mine, _lib._lib = _lib._lib, self.L

    def __exit__(self, *exc):
        from hifir_amd import _lib

        _lib._lib = self.mine


def _batch(n, width, cplx, seed=11):
    rng = np.random.default_rng(seed + width)
    B = rng.uniform(-1, 1, size=(n, width))
    if cplx:
        B = B + 1j * rng.uniform(-1, 1, size=(n, width))
    if width > NAN_COL:
        B[:, ZERO_COL] = 0.0
        B[:, NAN_COL] = np.nan
    return np.ascontiguousarray(B)


def _arrays(out):
    """the arrays of one call's return value, device tensors copied to the host"""
    out = out if isinstance(out, tuple) else (out,)
    return [o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o) for o in out]


def identity_outputs():
    """every output array of the entries the read-back path serves (X, flags, iters, sweeps, outer, relres, lambda, res, info3,
    ranks, the null-space basis and its residuals), on the small hierarchies of the GPU tests, through the host and the
    device-pointer form of each entry -> [(label, [arrays])], in a fixed order, from the library being served"""
    import torch

    import hifir_amd
    import lobpcg_gen_util
    import lobpcg_util
    from krylov_edges_util import csr_of, perturbed
    from test_gpu_pcg import _phase_similarity
    from util import load_hier

    got = []

    def forms(label, call, B):
        got.append((label + " host", _arrays(call(B))))
        got.append((label + " dev", _arrays(call(torch.from_numpy(B).cuda()))))
        torch.cuda.synchronize()

    def handle(levels, A, mass=None):
        M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
        M.set_matrix(A.indptr, A.indices, A.data)
        if mass is not None:
            M.set_mass_matrix(mass.indptr, mass.indices, mass.data)
        return M

    for name, real in (("cd2d_48", True), ("young1c", False)):  # general pairs: the GMRES family and the refinement
        levels, d = load_hier(name)
        M = handle(levels, perturbed(d, 0.05, real=real))
        for width in WIDTHS:
            B = _batch(len(d["b"]), width, not real)
            tag = "%s w%d " % (name, width)
            for restart in RESTARTS:
                forms(tag + "gmres(%d)" % restart, lambda b: M.gmres(b, restart=restart, rtol=1e-9, maxit=40), B)
                got.append((tag + "fgmres(%d)" % restart, _arrays(M.fgmres(B, restart=restart, rtol=1e-9, maxit=6))))
                forms(tag + "gmres_ir(%d)" % restart, lambda b: M.gmres_ir(b, restart=restart, max_outer=3, inner_maxit=40), B)
            forms(tag + "hifir", lambda b: M.hifir(b, 4), B)
            forms(tag + "hifir bounded", lambda b: M.hifir(b, 8, betas=(2e-3, 0.5)), B)
        M.close()
    for fixture in ("p2d_32_symm", "p2d_32_symm_z"):  # Hermitian pairs: PCG, the block methods, LOBPCG
        Cs = lobpcg_util.case(fixture)
        M = handle(Cs.levels, Cs.A, lobpcg_gen_util.mass_of(fixture))
        for width in WIDTHS:
            B = _batch(Cs.n, width, Cs.cplx)
            tag = "%s w%d " % (fixture, width)
            forms(tag + "pcg", lambda b: M.pcg(b, rtol=1e-8, maxit=30), B)
            for block in (16, 64):
                forms(tag + "bcg(%d)" % block, lambda b: M.bcg(b, block=block, rtol=1e-8, maxit=30), B)
            forms(tag + "bgcr", lambda b: M.bgcr(b, block=16, restart=5, rtol=1e-8, maxit=30), B)
        for k, nev in ((1, 1), (5, 5), (16, 13)):
            X0 = lobpcg_util.start_block(Cs.n, k, cplx=Cs.cplx)
            for entry in (M.lobpcg, M.lobpcg_gen):
                def run(x0):
                    return entry(X0=x0, nev=nev, tol=1e-8, maxit=8) + (M.last_lobpcg_info,)

                forms("%s k%d %s" % (fixture, k, entry.__name__), run, X0)
                got.append(("%s k%d %s generated" % (fixture, k, entry.__name__),
                            _arrays(entry(k=k, nev=nev, seed=3, tol=1e-8, maxit=8) + (M.last_lobpcg_info,))))
        M.close()
    levels, d = load_hier("twobody_symm")  # a singular pair and its complex twin: the null-space search
    A = csr_of(d)
    A.sort_indices()
    lz, Az, _ = _phase_similarity(levels, A)
    Az = Az.tocsr()
    Az.sort_indices()
    for tag, lv, Am in (("twobody_symm", levels, A), ("twobody_symm_z", lz, Az)):
        M = handle(lv, Am)
        for trans in (False, True):
            Q, resid, info = M.find_nullspace(tol=1e-8, rtol=1e-10, trans=trans)
            basis = M.nsp_basis(trans=trans)
            got.append(("%s find_nullspace trans=%d" % (tag, trans),
                        [Q, resid, np.array([info[key] for key in sorted(info)]), Q[:, :0] if basis is None else basis]))
        M.close()
    return got


def identity(parent):
    """-> {"bytes_compared", "differing_bytes", "arrays", "differing"}: identity_outputs() of this build against the parent's"""
    mine = identity_outputs()
    with serving(parent):
        import hifir_amd

        assert hifir_amd.lib() is parent
        theirs = identity_outputs()
    assert [label for label, _ in mine] == [label for label, _ in theirs]
    total = differing = arrays = 0
    where = []
    for (label, a), (_, b) in zip(mine, theirs):
        assert len(a) == len(b), label
        for i, (x, y) in enumerate(zip(a, b)):
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape, (label, i)
            bx, by = np.frombuffer(x.tobytes(), np.uint8), np.frombuffer(y.tobytes(), np.uint8)
            nd = int((bx != by).sum())
            total, differing, arrays = total + bx.size, differing + nd, arrays + 1
            if nd:
                where.append("%s [%d]: %d of %d bytes" % (label, i, nd, bx.size))
    return {"bytes_compared": total, "differing_bytes": differing, "arrays": arrays, "calls": len(mine), "differing": where}


def _five(pairs, parent_first=False):
    """{name: (call of this build, call of the parent's)} -> {name: {ms, repeats, parent_ms, parent_repeats, parent_min_max,
    within_parent_spread}}, the two builds taking turns, REPEATS figures each, the medians compared"""
    out = {}
    for name, (mine, theirs) in pairs.items():
        a, b = [], []
        for _ in range(REPEATS):
            if parent_first:
                b.append(theirs())
            a.append(mine())
            if not parent_first:
                b.append(theirs())
        med = float(np.median(a))
        out[name] = {"ms": med, "repeats": a, "parent_ms": float(np.median(b)), "parent_repeats": b,
                     "parent_min_max": [min(b), max(b)], "within_parent_spread": bool(min(b) <= med <= max(b)),
                     "not_slower_than_parent_max": bool(med <= max(b))}
        print(name, json.dumps(out[name]), flush=True)
    return out


def speed(parent, parent_first=False):
    """GMRES(30) ms per inner step, GMRES-IR with the defaults and LOBPCG ms per step on the 1M-row Poisson workload, this build
    and the parent's in the same process on handles made from the same factorization.  parent_first: the parent's handle is
    made first and goes first in every pair of repeats (where a handle's buffers land moves a figure by more than the repeats
    of one handle spread: a comparison wants both orders)"""
    import torch

    import hifir_amd
    from dev_lobpcg_gen import HI, K, LO, NEV, start_block
    from oracle import ref
    from util import poisson2d

    A = poisson2d(1000)

    def handles(params):
        levels = ref.RefHIF(A.indptr, A.indices, A.data, *params).levels()
        both = []
        for L in libs[::-1] if parent_first else libs:
            with serving(L):
                M = hifir_amd.HIF.from_levels(levels, max_nrhs=64)
                M.set_matrix(A.indptr, A.indices, A.data)
            both.append((M, L))
        return both[::-1] if parent_first else both  # (this build's, the parent's)

    def on(L, fn):
        with serving(L):
            return fn()

    def close(Ms):
        for M, L in Ms:
            on(L, M.close)

    libs = (hifir_amd.lib(), parent)
    res = {}
    Ms = handles(())
    B = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, size=(N, NC))).cuda()

    def gmres_step(M, L):
        def one():
            t1, _ = timed(lambda: M.gmres(B, restart=30, rtol=1e-300, maxit=1))
            t30, _ = timed(lambda: M.gmres(B, restart=30, rtol=1e-300, maxit=30))
            return (t30 - t1) / 29
        return lambda: on(L, one)

    def gmres_ir(M, L):
        return lambda: on(L, lambda: timed(lambda: M.gmres_ir(B))[0])

    for M, L in Ms[::-1] if parent_first else Ms:  # warm-up: buffers and the apply's graph
        on(L, lambda: (M.gmres(B, restart=30, rtol=1e-300, maxit=2), M.gmres_ir(B, max_outer=1)))
    res.update(_five({"gmres30_ms_per_inner_step": [gmres_step(M, L) for M, L in Ms],
                      "gmres_ir_defaults_ms": [gmres_ir(M, L) for M, L in Ms]}, parent_first))
    out = on(libs[0], lambda: Ms[0][0].gmres_ir(B))
    res["gmres_ir_defaults_ms"]["flags_outer_iters"] = [sorted(set(o.tolist())) for o in out[1:4]]
    close(Ms)
    del B
    Ms = handles((ref.make_params(is_symm=1),))
    X0 = start_block()

    def lobpcg_step(M, L):
        def one():
            t_lo, _ = timed(lambda: M.lobpcg(X0=X0, nev=NEV, tol=1e-300, maxit=LO))
            t_hi, _ = timed(lambda: M.lobpcg(X0=X0, nev=NEV, tol=1e-300, maxit=HI))
            return (t_hi - t_lo) / (HI - LO)
        return lambda: on(L, one)

    for M, L in Ms[::-1] if parent_first else Ms:
        on(L, lambda: M.lobpcg(X0=X0, nev=NEV, tol=1e-300, maxit=2))
    res.update(_five({"lobpcg_k%d_ms_per_step" % K: [lobpcg_step(M, L) for M, L in Ms]}, parent_first))
    close(Ms)
    return res


def against_parent(lib_path, out_dir, what, parent_first):
    import hashlib

    import torch  # noqa: F401  (before either library, as in measure())
    from dev_blockcg import stamp

    parent = load_library(lib_path)
    path = os.path.join(out_dir, "readback_refactor.json")
    res = json.load(open(path)) if os.path.exists(path) else {}
    res.update(stamp=stamp(), parent_lib_sha256=hashlib.sha256(open(lib_path, "rb").read()).hexdigest())
    if what in ("identity", "both"):
        res["identity"] = identity(parent)
        print(json.dumps(res["identity"], indent=1), flush=True)
    if what in ("speed", "both"):
        key = "speed_parent_first" if parent_first else "speed"
        res[key] = speed(parent, parent_first)
        print(json.dumps(res[key], indent=1), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    if "identity" in res and res["identity"]["differing_bytes"]:
        sys.exit("outputs differ from the parent library's")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace-steps", type=int)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--parent-lib")
    ap.add_argument("--what", choices=("identity", "speed", "both"), default="both")
    ap.add_argument("--parent-first", action="store_true")
    a = ap.parse_args()
    if a.kernel_stats:
        kernel_stats(a.kernel_stats)
    elif a.trace_steps:
        trace(a.trace_steps)
    elif a.parent_lib:
        against_parent(a.parent_lib, a.out or ".", a.what, a.parent_first)
    else:
        measure(a.out or ".")
