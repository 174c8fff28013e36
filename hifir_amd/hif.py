"""class HIF -- Python mirror of hif::HIF<ValueType,int> (reference src/hif/builder.hpp:109) for the
apply path, over the C ABI.  The names and argument meaning follow the reference:

  reference                                   here
  HIF::solve(b, x, trans=false, r=0)   :410   HIF.solve(b, rank=0) -> x
  HIF::solve_mrhs<Nrhs>(b, x, r)       :434   HIF.solve_mrhs(B, rank=0) -> X      (B is [n][nrhs])
  HIF::hifir(A, b, N, x, trans, r)     :459   HIF.hifir(b, N, rank=-1) -> x
  HIF::hifir(A, b, N, betas, x, ...)   :482   HIF.hifir(b, N, betas=(lo, hi)) -> (x, iters, flag)
  HIF::levels()/nnz()/rank()/schur_*   :141-190  same names

numpy arrays use the host-pointer entry points; torch CUDA tensors (device memory is the only thing
torch is used for) use the device-pointer entry points and are not synchronized.
Errors follow the reference convention (status code + message, libhifir.cpp:34-53): a non-zero
HifAmdStatus raises HifAmdError carrying the code and the library's message.
"""
import ctypes as C
import os

import numpy as np

from ._lib import lib

STATUS = {0: "HIFAMD_SUCCESS", 1: "HIFAMD_NULL_OBJ", 2: "HIFAMD_MISMATCHED_SIZES", 3: "HIFAMD_BAD_PREC",
          4: "HIFAMD_HIFIR_ERROR"}


OP_S, OP_SH, OP_M, OP_MH = 0, 1, 2, 3  # HifAmdOp == LhfOperationType (libhifir.h:159-164)
RESID_WORKING, RESID_COMPENSATED = 0, 1  # HIFAMD_RESID_*: how b - A x is formed (hifamd_set_residual_precision)
ZOP_TAIL, ZOP_TOP = 1, 2  #HIFAMD_ZOP_*: explicit operators a complex handle forms on request (hifamd_set_complex_operators)


class HifAmdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code
        self.msg = msg


def _check(code):
    if code != 0:
        m = lib().hifamd_last_error()
        raise HifAmdError(code, m.decode() if m else "")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _np_dtype_of(t):
    import torch

    return {torch.float64: np.dtype(np.float64), torch.complex128: np.dtype(np.complex128)}.get(t.dtype)


class HIF:
    """A multilevel preconditioner resident on one MI355X."""

    def __init__(self, dtype=np.float64, device=-1, complex_operators=0):
        """complex_operators: ZOP_TAIL | ZOP_TOP -- a complex handle forms the tail operator / the combined top operators
        that real handles always have (hifamd_set_complex_operators; 0: the default plan of complex handles)."""
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.complex128)):
            raise HifAmdError(3, "only float64 and complex128 hierarchies are supported")
        self._h = C.c_void_p()
        _check(lib().hifamd_create(0 if self.dtype == np.float64 else 1, device, C.byref(self._h)))
        self._A = None
        if complex_operators:
            self.set_complex_operators(complex_operators)

    def set_complex_operators(self, flags):
        """Before the first add_level, complex handles only (hifamd_set_complex_operators)."""
        _check(lib().hifamd_set_complex_operators(self._h, int(flags)))

    # ---- construction --------------------------------------------------------------------------
    @classmethod
    def from_levels(cls, levels, max_nrhs=64, rrqr_cond=0.0, device=-1, dtype=None, complex_operators=0):
        """levels: list of dicts with the fields of hif::Prec (alg/Prec.hpp:309-323), CCS matrices:
        m, n, {L,U,E,F}_{colptr,rowind,vals}, d, s, t, p, q_inv (+ p_inv, q), and on the last one
        optionally dense_n, dense (unfactored column-major Schur complement); dense_symm (+ spd) marks the block of
        a hierarchy factorized with is_symm, whose last level is the reference's SYEIG solver."""
        if dtype is None:
            cplx = any(np.iscomplexobj(lv["L_vals"]) or np.iscomplexobj(lv["d"]) or np.iscomplexobj(lv["E_vals"])
                       for lv in levels)
            dtype = np.complex128 if cplx else np.float64
        self = cls(dtype, device, complex_operators)
        for lv in levels:
            self.add_level(lv)
        last = levels[-1]
        if int(last.get("dense_n", 0)) > 0:
            if int(last.get("dense_lup", 0)):
                self.set_dense_lup(last["dense"])
            elif int(last.get("dense_symm", 0)):
                self.set_dense_symm(last["dense"], int(last.get("spd", 0)))
            else:
                self.set_dense(last["dense"], rrqr_cond)
        self.finalize(max_nrhs)
        return self

    def save(self, path, analysis=False):
        """Write the imported hierarchy (the add_level / set_dense arguments) to a file (hifamd_save).  analysis=True
        appends the host analysis of every level (hifamd_save_ex, HIFAMD_SAVE_ANALYSIS): a load under the same planner
        options adopts it instead of analyzing again (stats_ext()["analysis_cached_levels"])."""
        _check(lib().hifamd_save_ex(self._h, os.fsencode(path), 1 if analysis else 0))

    @classmethod
    def load(cls, path, max_nrhs=64, device=-1, complex_operators=0):
        """Read a hierarchy written by save() and ship it to the device (hifamd_load_ex + finalize).  The file does not
        hold the complex_operators of the handle that wrote it: they are the reader's choice."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self._A = None
        _check(lib().hifamd_load_ex(os.fsencode(path), device, int(complex_operators), C.byref(self._h)))
        with open(path, "rb") as f:
            f.seek(8)
            self.dtype = np.dtype(np.complex128 if int.from_bytes(f.read(8), "little") == 1 else np.float64)
        if max_nrhs:
            self.finalize(max_nrhs)
        return self

    def add_level(self, lv):
        dt = self.dtype
        m, n = int(lv["m"]), int(lv["n"])
        mats = []
        for k in "LUEF":
            mats += [np.ascontiguousarray(lv[k + "_colptr"], dtype=np.int64),
                     np.ascontiguousarray(lv[k + "_rowind"], dtype=np.int32),
                     np.ascontiguousarray(lv[k + "_vals"], dtype=dt)]
        f_ncols = len(mats[9]) - 1 if (n - m) else 0
        if f_ncols and mats[9][-1] == 0 and len(mats[9]) - 1 != n - m:
            f_ncols = 0
        d = np.ascontiguousarray(lv["d"], dtype=dt)
        s = np.ascontiguousarray(lv["s"], dtype=np.float64)
        t = np.ascontiguousarray(lv["t"], dtype=np.float64)
        perms = [None if lv.get(k) is None else np.ascontiguousarray(lv[k], dtype=np.int32)
                 for k in ("p", "p_inv", "q", "q_inv")]
        _check(lib().hifamd_add_level(self._h, m, n, *[_p(a) for a in mats[:9]], f_ncols, *[_p(a) for a in mats[9:]],
                                      _p(d), _p(s), _p(t), *[_p(a) for a in perms]))

    def set_dense(self, mat_colmajor, rrqr_cond=0.0):
        mat = np.ascontiguousarray(mat_colmajor, dtype=self.dtype).ravel()
        nd = int(round(np.sqrt(mat.size)))
        _check(lib().hifamd_set_dense(self._h, nd, _p(mat), float(rrqr_cond)))

    def set_dense_symm(self, mat_colmajor, spd=0):
        """Last level of a symmetric factorization (Prec::symm_dense_solver, SYEIG): eigendecomposition on the host."""
        mat = np.ascontiguousarray(mat_colmajor, dtype=self.dtype).ravel()
        nd = int(round(np.sqrt(mat.size)))
        _check(lib().hifamd_set_dense_symm(self._h, nd, _p(mat), int(spd)))

    def set_dense_lup(self, mat_colmajor):
        """Last level of a reference built with HIF_DENSE_MODE=0 (LU with partial pivoting, small_scale/LUP.hpp)."""
        mat = np.ascontiguousarray(mat_colmajor, dtype=self.dtype).ravel()
        nd = int(round(np.sqrt(mat.size)))
        _check(lib().hifamd_set_dense_lup(self._h, nd, _p(mat)))

    def finalize(self, max_nrhs=64):
        _check(lib().hifamd_finalize(self._h, int(max_nrhs)))
        # (the host copy is sealed at import and verified here, DESIGN 8: a copy that changed behind the library's back and
        #  was rebuilt is worth a Python warning as well -- pytest lists those even for tests that pass)
        rep = self.stats_ext().get("host_copy_repairs", 0.0)
        if rep:
            import warnings

            warnings.warn("hifir_amd: %d array(s) of the host copy had changed between add_level and finalize and were "
                          "rebuilt from the imported arrays (details on stderr)" % int(rep), RuntimeWarning)

    def set_matrix(self, indptr, indices, vals):
        """Attach the user's CRS matrix for iterative refinement (what lhf?Setup keeps, libhifir.cpp:413)."""
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        v = np.ascontiguousarray(vals, dtype=self.dtype)
        _check(lib().hifamd_set_matrix(self._h, len(ip) - 1, _p(ip), _p(ix), _p(v)))
        self._A = True

    def set_mass_matrix(self, indptr, indices, vals):
        """Attach the CRS mass matrix B of the generalized eigenproblem A x = lambda B x (hifamd_set_mass_matrix; lobpcg_gen).
        Arguments and checks of set_matrix; B is not checked for being Hermitian or positive definite."""
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        v = np.ascontiguousarray(vals, dtype=self.dtype)
        _check(lib().hifamd_set_mass_matrix(self._h, len(ip) - 1, _p(ip), _p(ix), _p(v)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().hifamd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- queries (builder.hpp:141-190) ------------------------------------------------------------
    def nrows(self):
        return lib().hifamd_nrows(self._h)

    ncols = nrows

    def levels(self):
        return lib().hifamd_levels(self._h)

    def nnz(self):
        return lib().hifamd_nnz(self._h)

    def schur_size(self):
        return lib().hifamd_schur_size(self._h)

    def schur_rank(self):
        return lib().hifamd_schur_rank(self._h)

    def rank(self):
        return self.nrows() - (self.schur_size() - self.schur_rank()) if self.schur_size() else self.nrows()

    def stats(self):
        s = np.zeros(16)
        _check(lib().hifamd_stats(self._h, _p(s)))
        keys = ["sum_n", "sum_m", "nnz_LU", "nnz_EF", "dense_n", "B_mat", "B_vec", "wavefronts_L", "wavefronts_U",
                "launches", "sparse_levels", "bands", "band_workgroups", "finalize_s", "operator_bytes", "graph_capture_ms"]
        return {k: float(s[i]) for i, k in enumerate(keys)}

    def stats_ext(self):
        """Set-up cost and resident explicit operators (hifamd_stats_ext)."""
        s = np.zeros(32)
        k = lib().hifamd_stats_ext(self._h, _p(s), 32)
        keys = ["finalize_s", "graph_capture_ms", "bytes_inverses", "bytes_top", "bytes_tail", "tail_rows", "tail_level",
                "tail_probe_relerr", "tail_max_abs", "tail_rejected", "tail_probe_tol", "tail_max_growth",
                "analysis_cached_levels", "analysis_s", "arena_bytes", "arena_cols", "tile_bytes", "factor_bytes", "max_nrhs",
                "rows_not_stored_L", "rows_not_stored_U", "host_copy_repairs", "nsp_basis_bytes"]
        out = {key: float(s[i]) for i, key in enumerate(keys[:max(0, k)])}
        # component bands (slots 26 / 27): their components, and the workgroups that own more than one of them
        out.update({key: float(s[26 + i]) for i, key in enumerate(("cd_components", "cd_shared_workgroups")) if 26 + i < k})
        return out

    def complex_operators(self):
        """The flags of hifamd_set_complex_operators in force (hifamd_stats_ext slot 29; real handles: 0).  A method of its
        own, like ls_stats(): the keys of stats_ext() are counted by tests/test_nsp_basis_host.py."""
        s = np.zeros(32)
        k = lib().hifamd_stats_ext(self._h, _p(s), 32)
        return int(s[29]) if k > 29 else 0

    def ls_stats(self):
        """Sparse-own L bands that run with streamed sources (hifamd_stats_ext slots 23-25 and 28): rows streamed as sources,
        rows kept in LDS as dependent rows, rows of the source chunk (0: no band runs that way), most chunks of one component."""
        s = np.zeros(32)
        k = lib().hifamd_stats_ext(self._h, _p(s), 32)
        slots = {"ls_streamed_sources": 23, "ls_lds_rows": 24, "ls_chunk_rows": 25, "ls_max_chunks": 28}
        return {key: float(s[i]) if i < k else 0.0 for key, i in slots.items()}

    def level_stats(self, level):
        s = np.zeros(16)
        k = lib().hifamd_level_stats(self._h, int(level), _p(s), 16)
        if k < 0:
            raise HifAmdError(2, "no such level")
        keys = ["m", "n", "nnz_L", "nnz_U", "nnz_E", "nnz_F", "wavefronts_L", "wavefronts_U", "bands_L", "bands_U", "top_rows"]
        return {key: float(s[i]) for i, key in enumerate(keys[:k])}

    def launch_map(self):
        """(level, stage) of every kernel launch of the last batched apply, in launch order (hifamd_launch_map)."""
        k = lib().hifamd_launch_map(self._h, None, 0)
        o = np.zeros(max(k, 1), dtype=np.int32)
        lib().hifamd_launch_map(self._h, _p(o), int(k))
        return [(int(v) // 16, int(v) % 16) for v in o[:k]]

    def kernel_census(self, lower=False):
        """{kernel family: launches} of the last batched apply, forwards or transposed, summed over its lanes
        (hifamd_kernel_census).  lower=True: only the launches on a level >= 1.  Every family is present; the families and
        their order are the library's (hifamd_kernel_family_name)."""
        k = lib().hifamd_kernel_census(self._h, None, 0)
        if k <= 0:
            return {}
        o = np.zeros(k, dtype=np.int32)
        lib().hifamd_kernel_census(self._h, _p(o), int(k))
        nf = k // 2
        names = [lib().hifamd_kernel_family_name(f).decode() for f in range(nf)]
        return {name: int(o[(nf if lower else 0) + f]) for f, name in enumerate(names)}

    def level_bytes(self, nrhs):
        """B_alg(nrhs) of SURVEY 8(d) level by level and stage by stage: {level: {stage: bytes}} with the stage codes of
        launch_map(); the dense block's bytes sit at stage 4 of the level that owns it."""
        sv = np.dtype(self.dtype).itemsize
        si, sp, ss = 4, 8, 8
        st = self.stats()
        out = {}
        nlev = int(st["sparse_levels"])
        for l in range(nlev):
            q = self.level_stats(l)
            m, n = q["m"], q["n"]
            nm = n - m
            ldu = 2 * m * sv * nrhs + (q["nnz_L"] + q["nnz_U"]) * (sv + si) + m * sv + 2 * (m + 1) * sp  # one LDU solve
            out[l] = {
                1: 2 * n * sv * nrhs + n * (si + ss),  # S1: read + write n rows, p and s
                2: ldu,
                3: (m + 2 * nm) * sv * nrhs + q["nnz_E"] * (sv + si) + (nm + 1) * sp,
                4: (st["dense_n"] ** 2 * sv) if l == nlev - 1 else 0.0,
                5: (nm + 2 * m) * sv * nrhs + q["nnz_F"] * (sv + si) + (m + 1) * sp,
                6: ldu,
                7: 2 * n * sv * nrhs + n * (si + ss),  # S7: read + write n rows, q_inv and t
            }
        tot = sum(sum(v.values()) for v in out.values())
        ref = self.algorithmic_bytes(nrhs)
        assert abs(tot - ref) <= 1e-6 * ref, (tot, ref)
        return out

    def algorithmic_bytes(self, nrhs):
        """B_alg(nrhs) = B_mat + nrhs * B_vec of SURVEY 8(d), for the hierarchy actually resident."""
        st = self.stats()
        return st["B_mat"] + nrhs * st["B_vec"]

    def stage_bytes(self, nrhs):
        """The same B_alg split by stage group (SURVEY 8(d) terms): which kernels stream which bytes.
        permute = S1 + S7 (k_gather_scale / k_scatter_scale), ldu = S2 + S6 (k_trsv_* / k_thin_update /
        k_tri_gemm_d), schur = S3 + S5 (k_spmm_epi), dense = last-level operators."""
        st = self.stats()
        sv = np.dtype(self.dtype).itemsize
        si, sp, ss = 4, 8, 8
        n, m, L = st["sum_n"], st["sum_m"], st["sparse_levels"]
        nm = n - m
        out = {
            "permute": 4 * n * sv * nrhs + n * (2 * si + 2 * ss),
            "ldu": 4 * m * sv * nrhs + 2 * st["nnz_LU"] * (sv + si) + 2 * m * sv + 4 * (m + L) * sp,
            "schur": (3 * m + 3 * nm) * sv * nrhs + st["nnz_EF"] * (sv + si) + (n + 2 * L) * sp,
            "dense": st["dense_n"] ** 2 * sv,
        }
        assert abs(sum(out.values()) - self.algorithmic_bytes(nrhs)) <= 1e-9 * self.algorithmic_bytes(nrhs)
        return out

    def level_schedule(self, level, which):
        """(order, wf_ptr) of the L (which=0) or U (which=1) factor of a level."""
        nwf = C.c_int64()
        _check(lib().hifamd_level_schedule(self._h, level, which, C.byref(nwf), None, None))
        stt = np.zeros(16)
        lib().hifamd_stats(self._h, _p(stt))
        # m is not exported separately: take it from wf_ptr's last entry
        wf = np.zeros(nwf.value + 1, dtype=np.int64)
        _check(lib().hifamd_level_schedule(self._h, level, which, None, None, _p(wf)))
        order = np.zeros(int(wf[-1]), dtype=np.int32)
        _check(lib().hifamd_level_schedule(self._h, level, which, None, _p(order), None))
        return order, wf

    # ---- argument checks of the device-pointer entry points ------------------------------------------
    def _dev_block(self, T, what, shape=None):
        """A CUDA tensor handed to a *_dev entry point must be what the kernels assume: on the handle's device, of
        the handle's value type, [nrows][nrhs] with unit column stride.  Anything else would be an out-of-bounds
        device access (a GPU memory fault aborts the process), so it is refused here with MISMATCHED_SIZES."""
        if not _is_torch(T) or not T.is_cuda:
            raise HifAmdError(2, f"{what}: expected a CUDA tensor")
        dev = lib().hifamd_device(self._h)
        if dev >= 0 and T.device.index != dev:
            raise HifAmdError(2, f"{what}: tensor lives on cuda:{T.device.index}, the hierarchy on cuda:{dev}")
        # (`is None` first: numpy reads a comparison with None as one with its default dtype, float64, so on a real handle
        # `None != self.dtype` is False and a float32 tensor would pass, to be read as float64 past its end)
        if _np_dtype_of(T) is None or _np_dtype_of(T) != self.dtype:
            raise HifAmdError(2, f"{what}: dtype {T.dtype} does not match the hierarchy's {self.dtype}")
        if T.dim() != 2 or T.shape[0] != self.nrows() or T.shape[1] < 1:
            raise HifAmdError(2, f"{what}: expected an [nrows][nrhs] block, got {tuple(T.shape)}")
        if T.stride(1) != 1 or T.stride(0) < T.shape[1]:
            raise HifAmdError(2, f"{what}: blocks must be row-interleaved (unit column stride)")
        if shape is not None and tuple(T.shape) != tuple(shape):
            raise HifAmdError(2, f"{what}: shape {tuple(T.shape)} differs from the input's {tuple(shape)}")
        return T

    def _host_out(self, X, like, what="x"):
        """A caller-supplied host output is written through its pointer: it must be exactly that buffer."""
        if X is None:
            return np.empty_like(like)
        if not isinstance(X, np.ndarray) or X.dtype != self.dtype or X.shape != like.shape or not X.flags.c_contiguous:
            raise HifAmdError(2, f"{what}: output must be a C-contiguous {self.dtype} array of shape {like.shape}")
        return X

    # ---- apply -----------------------------------------------------------------------------------
    def solve(self, b, x=None, trans=False, rank=0):
        """x = M^{-1} b, or x = M^{-H} b with trans=True (HIF::solve, builder.hpp:409-423)."""
        if _is_torch(b):
            return self.solve_mrhs(b.reshape(-1, 1), None if x is None else x.reshape(-1, 1), rank, trans=trans).reshape(-1)
        b = np.ascontiguousarray(b, dtype=self.dtype)
        if b.ndim != 1 or b.shape[0] != self.nrows():
            raise HifAmdError(2, "unmatched sizes")
        x = self._host_out(x, b)
        if trans:
            _check(lib().hifamd_apply_batch(self._h, OP_SH, _p(b), 1, _p(x), 1, 1, 1, None, int(rank), None))
        else:
            _check(lib().hifamd_solve(self._h, _p(b), _p(x), int(rank)))
        return x

    def solve_mrhs(self, B, X=None, rank=0, stream=None, trans=False):
        """X = M^{-1} B (trans: M^{-H} B) for an [n][nrhs] row-interleaved block (the layout of
        Array<std::array<T,Nrhs>>, CompressedStorage.hpp:2127); nrhs is a run-time value here."""
        op = OP_SH if trans else OP_S
        if _is_torch(B):
            import torch

            self._dev_block(B, "B")
            if X is None:
                X = torch.empty_like(B)
            self._dev_block(X, "X", B.shape)
            _check(lib().hifamd_apply_batch_dev(self._h, op, B.data_ptr(), B.stride(0), X.data_ptr(), X.stride(0),
                                               B.shape[1], int(rank), stream))
            return X
        B = np.ascontiguousarray(B, dtype=self.dtype)
        if B.ndim != 2 or B.shape[0] != self.nrows():
            raise HifAmdError(2, "unmatched sizes")
        X = self._host_out(X, B, "X")
        if trans:
            _check(lib().hifamd_apply_batch(self._h, op, _p(B), B.shape[1], _p(X), X.shape[1], B.shape[1], 1, None,
                                           int(rank), None))
        else:
            _check(lib().hifamd_solve_batch(self._h, _p(B), B.shape[1], _p(X), X.shape[1], B.shape[1], int(rank)))
        return X

    def set_nsp_const(self, start=0, end=-1, trans=False):
        """Constant-mode null-space filter of solve() (HIF::nsp; trans: HIF::nsp_tran): rows [start, end) of
        every solution lose their mean; start > end >= 0 removes the filter."""
        _check(lib().hifamd_set_nsp_const(self._h, OP_SH if trans else OP_S, int(start), int(end)))

    def set_nsp_basis(self, V, trans=False):
        """Basis mode of the null-space filter (hifamd_set_nsp_basis): V, (n,) or (n, k) with 1 <= k <= 16, spans the
        null space; after every solve (trans: every M^{-H} solve), also inside hifir / gmres / bicgstab, each column x
        becomes x - Q (Q^H x) with Q an orthonormal basis of span(V).  None removes it.  With a basis set, pcg() and
        sqmr() run projected on the complement of span(Q)."""
        op = OP_SH if trans else OP_S
        if V is None:
            _check(lib().hifamd_set_nsp_basis(self._h, op, 0, None, 0))
            return
        V = np.asarray(V)
        if V.ndim == 1:
            V = V.reshape(-1, 1)
        V = np.ascontiguousarray(V, dtype=self.dtype)
        if V.ndim != 2 or V.shape[0] != self.nrows():
            raise HifAmdError(2, "null-space basis: expected (n,) or (n, k)")
        _check(lib().hifamd_set_nsp_basis(self._h, op, V.shape[1], _p(V), V.shape[1]))

    def nsp_dim(self, trans=False):
        """Vectors of the basis filter in force (0: none, or constant mode)."""
        return int(lib().hifamd_nsp_dim(self._h, OP_SH if trans else OP_S))

    def find_nullspace(self, kmax=16, tol=1e-7, rtol=1e-10, restart=30, maxit=500, trans=False, install=True, X0=None,
                       seed=0, full_rank=False):
        """Find the null space of the attached matrix (trans: of A^H) on the device (hifamd_nsp_find): 16 probe columns
        x0, GMRES on A d = -A x0 to rtol, V = X0 + D ordered and orthonormalized, a column q accepted when
        ||A q||_2 <= tol ||A||_inf; `found` = the leading accepted columns, at most kmax.  rtol sqrt(n / nullity) has to
        stay below tol, and tol below sigma_min+(A) / ||A||_inf.  X0: (n, 16) host probes of the handle's dtype; None:
        generated on the device from `seed` (the generator of include/hifir_amd.h).  install: the found vectors become
        the basis filter (as set_nsp_basis would set them); nothing found leaves the filter in force as it was.
        Returns (Q (n, found), resid (16,) = ||A q_j|| / ||A||_inf per column, inf for a dropped one, info) with info =
        {"unconverged": probe columns whose GMRES did not converge, "iters": largest GMRES iteration count,
        "maybe_more": a column beyond kmax passed too, or found == 16, "nonfinite": something non-finite was met}."""
        n = self.nrows()
        kmax = int(kmax)
        if X0 is not None:
            if not isinstance(X0, np.ndarray) or X0.ndim != 2 or X0.shape != (n, 16):
                raise HifAmdError(2, "X0: expected an (n, 16) block of probe columns")
            X0 = np.ascontiguousarray(X0, dtype=self.dtype)
        Q = np.zeros((n, min(max(kmax, 1), 16)), dtype=self.dtype)
        resid = np.zeros(16)
        info = np.zeros(4, dtype=np.int32)
        found = C.c_int64(0)
        _check(lib().hifamd_nsp_find(self._h, OP_SH if trans else OP_S, kmax, float(tol), float(rtol), int(restart),
                                     int(maxit), -1 if full_rank else 0, _p(X0), 16, int(seed) & (2 ** 64 - 1),
                                     1 if install else 0, C.byref(found), _p(Q), Q.shape[1], _p(resid), _p(info)))
        keys = ("unconverged", "iters", "maybe_more", "nonfinite")
        return np.ascontiguousarray(Q[:, :found.value]), resid, {k: int(info[i]) for i, k in enumerate(keys)}

    def nsp_basis(self, trans=False):
        """The orthonormal basis of the basis filter in force, (n, k) (hifamd_nsp_get_basis); None when there is none
        (or the filter is in constant mode)."""
        op = OP_SH if trans else OP_S
        k = self.nsp_dim(trans)
        if k <= 0:
            return None
        Q = np.empty((self.nrows(), k), dtype=self.dtype)
        if lib().hifamd_nsp_get_basis(self._h, op, _p(Q), k) != k:
            _check(4)
        return Q

    def nsp_filter(self, X, trans=False):
        """The filter in force (basis or constant mode) alone, in place, on X ((n,) or (n, nrhs); a C-contiguous host
        array of the handle's dtype, or a CUDA tensor, which is not synchronized); returns X.  No filter: X as it is."""
        op = OP_SH if trans else OP_S
        if _is_torch(X):
            X2 = self._dev_block(X.reshape(X.shape[0], -1), "X")
            if X2.data_ptr() != X.data_ptr():
                raise HifAmdError(2, "X: blocks must be row-interleaved (unit column stride)")
            _check(lib().hifamd_nsp_filter_batch_dev(self._h, op, X2.data_ptr(), X2.stride(0), X2.shape[1], None))
            return X
        if not isinstance(X, np.ndarray) or X.dtype != self.dtype or not X.flags.c_contiguous or X.ndim not in (1, 2) \
                or X.shape[0] != self.nrows():
            raise HifAmdError(2, f"X: expected a C-contiguous {self.dtype} array of shape (n,) or (n, nrhs)")
        nrhs = 1 if X.ndim == 1 else X.shape[1]
        _check(lib().hifamd_nsp_filter_batch(self._h, op, _p(X), nrhs, nrhs))
        return X

    def mmultiply(self, x, trans=False, rank=-1):
        """y = M x (trans: M^H x), the multilevel product HIF::mmultiply (builder.hpp:503-513) -- the inverse
        direction of solve().  x: [n] or [n][nrhs], host array or CUDA tensor."""
        op = OP_MH if trans else OP_M
        vec = (x.ndim == 1)
        if _is_torch(x):
            import torch

            X = self._dev_block(x.reshape(x.shape[0], -1), "x")
            Y = torch.empty_like(X)
            _check(lib().hifamd_apply_batch_dev(self._h, op, X.data_ptr(), X.stride(0), Y.data_ptr(), Y.stride(0),
                                               X.shape[1], int(rank), None))
        else:
            X = np.ascontiguousarray(x, dtype=self.dtype).reshape(x.shape[0], -1)
            Y = np.empty_like(X)
            _check(lib().hifamd_apply_batch(self._h, op, _p(X), X.shape[1], _p(Y), Y.shape[1], X.shape[1], 1, None,
                                           int(rank), None))
        return Y.reshape(-1) if vec else Y

    def spmv(self, X, Y=None, stream=None):
        """Y = A X on the device (torch CUDA tensors, [n][nrhs] or [n])."""
        import torch

        X2 = self._dev_block(X.reshape(X.shape[0], -1), "X")
        if Y is None:
            Y = torch.empty_like(X)
        Y2 = self._dev_block(Y.reshape(Y.shape[0], -1), "Y", X2.shape)
        _check(lib().hifamd_spmv_batch_dev(self._h, X2.data_ptr(), X2.stride(0), Y2.data_ptr(), Y2.stride(0),
                                          X2.shape[1], stream))
        return Y

    def hifir(self, b, N, betas=None, rank=-1, trans=False):
        """Iterative refinement (HIF::hifir, builder.hpp:459-489).  b: [n] or [n][nrhs].
        Without betas returns x; with betas returns (x, iters, flags) per column (ints for a vector).
        trans=True refines A^H x = b with M^{-H} (host arrays only)."""
        if trans:
            if _is_torch(b):
                raise HifAmdError(3, "hifir(trans=True) takes host arrays")
            vec = (b.ndim == 1)
            bt = None if betas is None else np.ascontiguousarray(betas, dtype=np.float64)
            B = np.ascontiguousarray(b, dtype=self.dtype).reshape(b.shape[0], -1)
            X = np.empty_like(B)
            st = np.zeros(2 * B.shape[1], dtype=np.int32)
            _check(lib().hifamd_apply_batch(self._h, OP_SH, _p(B), B.shape[1], _p(X), X.shape[1], B.shape[1], int(N),
                                           _p(bt), int(rank), _p(st)))
            x = X.reshape(-1) if vec else X
            if betas is None:
                return x
            it, fl = st[0::2].copy(), st[1::2].copy()
            return (x, int(it[0]), int(fl[0])) if vec else (x, it, fl)
        vec = (b.ndim == 1)
        bt = None if betas is None else np.ascontiguousarray(betas, dtype=np.float64)
        if _is_torch(b):
            import torch

            B = self._dev_block(b.reshape(b.shape[0], -1), "b")
            X = torch.empty_like(B)
            st = np.zeros(2 * B.shape[1], dtype=np.int32)
            _check(lib().hifamd_hifir_batch_dev(self._h, B.data_ptr(), B.stride(0), X.data_ptr(), X.stride(0),
                                               B.shape[1], int(N), _p(bt), int(rank), _p(st)))
        else:
            B = np.ascontiguousarray(b, dtype=self.dtype).reshape(b.shape[0], -1)
            X = np.empty_like(B)
            st = np.zeros(2 * B.shape[1], dtype=np.int32)
            _check(lib().hifamd_hifir_batch(self._h, _p(B), B.shape[1], _p(X), X.shape[1], B.shape[1], int(N), _p(bt),
                                           int(rank), _p(st)))
        x = X.reshape(-1) if vec else X
        if betas is None:
            return x
        it, fl = st[0::2].copy(), st[1::2].copy()
        return (x, int(it[0]), int(fl[0])) if vec else (x, it, fl)

    def _krylov(self, name, b, *lead, rtol, maxit, full_rank, mid=(), tail=()):
        """The batched solver hifamd_<name>_batch (host array) or hifamd_<name>_batch_dev (CUDA tensor) on all columns of
        b; lead are the solver's arguments ahead of rtol, mid those between rtol and maxit, tail those behind iters.
        Returns (x, flags, iters); ints for a vector."""
        vec = (b.ndim == 1)
        if _is_torch(b):
            import torch

            B = self._dev_block(b.reshape(b.shape[0], -1), "b")
            X = torch.empty_like(B)
            fn, io = getattr(lib(), "hifamd_%s_batch_dev" % name), (B.data_ptr(), B.stride(0), X.data_ptr(), X.stride(0))
        else:
            B = np.ascontiguousarray(b, dtype=self.dtype).reshape(b.shape[0], -1)
            X = np.empty_like(B)
            fn, io = getattr(lib(), "hifamd_%s_batch" % name), (_p(B), B.shape[1], _p(X), X.shape[1])
        fl = np.zeros(B.shape[1], dtype=np.int32)
        it = np.zeros(B.shape[1], dtype=np.int32)
        _check(fn(self._h, *io, B.shape[1], *lead, float(rtol), *mid, int(maxit), -1 if full_rank else 0, _p(fl), _p(it), *tail))
        if vec:
            return X.reshape(-1), int(fl[0]), int(it[0])
        return X, fl, it

    def gmres(self, b, restart=30, rtol=1e-6, maxit=500, full_rank=False):
        """Right-preconditioned restarted GMRES (the reference's examples/advanced/gmres.hpp:19-123),
        all columns of b ([n] or [n][nrhs], host array or CUDA tensor) in lock step on the device.
        Returns (x, flags, iters); ints for a vector."""
        return self._krylov("gmres", b, int(restart), rtol=rtol, maxit=maxit, full_rank=full_rank)

    # ---- extra-precise residuals ---------------------------------------------------------------------
    def set_residual_precision(self, mode):
        """How hifir / gmres / fgmres form b - A x (hifamd_set_residual_precision): RESID_WORKING (0) in working
        precision, RESID_COMPENSATED (1) as if in twice the working precision.  The default comes from
        HIFIR_AMD_RESIDUAL when the handle is created."""
        _check(lib().hifamd_set_residual_precision(self._h, int(mode)))

    def residual_precision(self):
        """The residual mode in force (hifamd_residual_precision)."""
        m = lib().hifamd_residual_precision(self._h)
        if m < 0:
            _check(1)
        return m

    def residual(self, B, X, trans=False, precise=None):
        """R = B - A X (trans: B - A^H X) on the device (hifamd_residual_batch / _dev).  B, X: [n] or [n][nrhs], both host
        arrays or both CUDA tensors (not synchronized).  precise: True compensated, False working precision, None the
        handle's mode."""
        op = OP_SH if trans else OP_S
        mode = -1 if precise is None else (1 if precise else 0)
        vec = (B.ndim == 1)
        if _is_torch(B) != _is_torch(X):
            raise HifAmdError(2, "residual: B and X must both be host arrays or both CUDA tensors")
        if _is_torch(B):
            import torch

            B2 = self._dev_block(B.reshape(B.shape[0], -1), "B")
            X2 = self._dev_block(X.reshape(X.shape[0], -1), "X", B2.shape)
            R = torch.empty((B2.shape[0], B2.shape[1]), dtype=B2.dtype, device=B2.device)
            _check(lib().hifamd_residual_batch_dev(self._h, op, B2.data_ptr(), B2.stride(0), X2.data_ptr(), X2.stride(0),
                                                  R.data_ptr(), R.stride(0), B2.shape[1], mode, None))
        else:
            B2 = np.ascontiguousarray(B, dtype=self.dtype).reshape(B.shape[0], -1)
            X2 = np.ascontiguousarray(X, dtype=self.dtype).reshape(X.shape[0], -1)
            if B2.shape[0] != self.nrows() or X2.shape != B2.shape:
                raise HifAmdError(2, "unmatched sizes")
            R = np.empty_like(B2)
            _check(lib().hifamd_residual_batch(self._h, op, _p(B2), B2.shape[1], _p(X2), X2.shape[1], _p(R), R.shape[1],
                                              B2.shape[1], mode))
        return R.reshape(-1) if vec else R

    def gmres_ir(self, b, restart=30, rtol=1e-14, inner_rtol=1e-6, max_outer=10, inner_maxit=500, full_rank=False):
        """GMRES-based iterative refinement (hifamd_gmres_ir_batch / _dev): outer residuals always compensated, every
        correction A d = r by right-preconditioned GMRES to inner_rtol.  b: [n] or [n][nrhs], host array or CUDA tensor.
        Returns (x, flags, outer, iters, relres) per column (scalars for a vector): flags 0 converged / 1 stagnated (x is
        the better of the last two iterates) / 2 reached max_outer; outer = corrections in x; iters = inner GMRES
        iterations; relres = the compensated ||b - A x|| / ||b|| of the returned x."""
        vec = (b.ndim == 1)
        if _is_torch(b):
            import torch

            B = self._dev_block(b.reshape(b.shape[0], -1), "b")
            X = torch.empty_like(B)
            fn, io = lib().hifamd_gmres_ir_batch_dev, (B.data_ptr(), B.stride(0), X.data_ptr(), X.stride(0))
        else:
            B = np.ascontiguousarray(b, dtype=self.dtype).reshape(b.shape[0], -1)
            X = np.empty_like(B)
            fn, io = lib().hifamd_gmres_ir_batch, (_p(B), B.shape[1], _p(X), X.shape[1])
        fl, ou, it = (np.zeros(B.shape[1], dtype=np.int32) for _ in range(3))
        rr = np.zeros(B.shape[1])
        _check(fn(self._h, *io, B.shape[1], int(restart), float(rtol), float(inner_rtol), int(max_outer), int(inner_maxit),
                  -1 if full_rank else 0, _p(fl), _p(ou), _p(it), _p(rr)))
        if vec:
            return X.reshape(-1), int(fl[0]), int(ou[0]), int(it[0]), float(rr[0])
        return X, fl, ou, it, rr

    def is_hermitian(self):
        """True when M^{-1} of the imported hierarchy is Hermitian (hifamd_hermitian: exact test on the host copy, every
        level U_B == L_B^H, F == E^H, s == t, p == q, Im d == 0, last level SYEIG or absent).  Needs no finalize, no GPU."""
        h = lib().hifamd_hermitian(self._h)
        if h < 0:
            _check(1)
        return h == 1

    def pcg(self, b, rtol=1e-6, maxit=500, full_rank=False):
        """Preconditioned CG (x0 = 0) for a Hermitian positive-definite pair (A, M), all columns of b ([n] or
        [n][nrhs], host array or CUDA tensor) in lock step on the device.  Needs set_matrix and is_hermitian().
        Returns (x, flags, iters); ints for a vector.  flags: 0 converged, 1 breakdown, 2 reached maxit."""
        return self._krylov("pcg", b, rtol=rtol, maxit=maxit, full_rank=full_rank)

    def bcg(self, b, block=64, rtol=1e-6, maxit=500, deftol=1e-12, full_rank=False):
        """Breakdown-free block CG (x0 = 0) for a Hermitian positive-definite pair (A, M) (hifamd_bcg_batch / _dev): the
        columns of b ([n] or [n][nrhs], host array or CUDA tensor) are cut into tiles of `block` <= 64, and the columns of a
        tile share one block Krylov space; dependent, duplicate and zero columns shrink the block (a pivoted Cholesky that
        drops pivots <= deftol) instead of breaking it down.  Needs set_matrix and is_hermitian().  Returns
        (x, flags, iters, ranks); ints for a vector, ranks always an array: per tile its rank after the start and during
        its last step.  flags: 0 converged, 1 breakdown or a non-finite column, 2 reached maxit; iters: the steps of the
        column's tile.  A column's result depends on the columns it shares a tile with."""
        ntile = -(-(1 if b.ndim == 1 else int(b.shape[1])) // max(int(block), 1))
        ranks = np.zeros(2 * max(ntile, 1), dtype=np.int32)
        x, fl, it = self._krylov("bcg", b, int(block), rtol=rtol, maxit=maxit, full_rank=full_rank, mid=(float(deftol),),
                                 tail=(_p(ranks),))
        return x, fl, it, ranks

    def lobpcg(self, k=8, nev=None, X0=None, seed=0, tol=1e-8, maxit=200, deftol=1e-12, full_rank=False):
        """LOBPCG for the nev smallest eigenpairs of the Hermitian matrix of set_matrix, preconditioned by the hierarchy
        (hifamd_lobpcg / _dev): a block of k <= 16 candidates (nev <= k, default k; the others are guard columns), started
        from X0 ([n][k], host array or CUDA tensor; its width is k) or from the generated block of `seed`.  A column is
        converged when ||A x - lambda x||_2 <= tol ||A||_inf.  Needs set_matrix and is_hermitian(); with a basis filter
        (set_nsp_basis) it returns the smallest eigenvalues on the complement of span(Q).  Returns
        (lam, X, res, flags, steps): lam [k] ascending, X [n][k] orthonormal (a CUDA tensor where X0 is one), res [k] the last
        residuals, flags [k] 0 converged / 1 breakdown / 2 not converged at maxit, steps (one apply plus one SpMM each);
        last_lobpcg_info keeps the call's info3 (steps, rank of the last basis, largest Jacobi sweep count)."""
        return self._lobpcg("hifamd_lobpcg", k, nev, X0, seed, tol, maxit, deftol, full_rank)

    def lobpcg_gen(self, k=8, nev=None, X0=None, seed=0, tol=1e-8, maxit=200, deftol=1e-12, full_rank=False):
        """LOBPCG for the nev smallest eigenpairs of the Hermitian definite pencil A x = lambda B x, A of set_matrix and B of
        set_mass_matrix, preconditioned by the hierarchy (hifamd_lobpcg_gen / _dev).  Arguments and returns of lobpcg; X comes
        back with X^H B X = I, and a column is converged when ||A x - lambda B x||_2 <= tol (||A||_inf + |lambda| ||B||_inf)
        ||x||_2, the normwise backward error of the pair.  Needs set_matrix, set_mass_matrix and is_hermitian(), and runs
        under no null-space filter (neither set_nsp_const nor set_nsp_basis: the projector would have to be B-orthogonal)."""
        return self._lobpcg("hifamd_lobpcg_gen", k, nev, X0, seed, tol, maxit, deftol, full_rank)

    def _lobpcg(self, entry, k, nev, X0, seed, tol, maxit, deftol, full_rank):
        dev = X0 is not None and _is_torch(X0)
        if X0 is not None:
            if dev:
                import torch

                X0 = self._dev_block(X0, "X0")
                X = torch.empty((X0.shape[0], X0.shape[1]), dtype=X0.dtype, device=X0.device)
                io0, io1 = (X0.data_ptr(), X0.stride(0)), (X.data_ptr(), X.stride(0))
            else:
                X0 = np.ascontiguousarray(X0, dtype=self.dtype)
                if X0.ndim != 2 or X0.shape[0] != self.nrows():
                    raise HifAmdError(2, "X0: expected an [nrows][k] block")
                io0 = (_p(X0), X0.shape[1])
            k = int(X0.shape[1])
        else:
            io0 = (None, 0)
        if not dev:
            X = np.empty((self.nrows(), max(int(k), 1)), dtype=self.dtype)
            io1 = (_p(X), X.shape[1])
        nev = int(k) if nev is None else int(nev)
        lam, res = np.zeros(max(int(k), 1)), np.zeros(max(int(k), 1))
        fl, info = np.zeros(max(int(k), 1), dtype=np.int32), np.zeros(3, dtype=np.int32)
        fn = getattr(lib(), entry + "_dev" if dev else entry)
        _check(fn(self._h, int(k), nev, *io0, int(seed), float(tol), float(deftol), int(maxit), -1 if full_rank else 0, _p(lam),
                  *io1, _p(res), _p(fl), _p(info)))
        self.last_lobpcg_info = info
        return lam, X, res, fl, int(info[0])

    def _eig_block(self, V, name, like_dev):
        """V as an [nrows][c] block the C entries take: -> (block, pointer, row stride); like_dev: it must be a CUDA tensor"""
        if like_dev != _is_torch(V):
            raise HifAmdError(2, f"{name}: host arrays and CUDA tensors cannot be mixed in one call")
        if like_dev:
            V = self._dev_block(V, name)
            return V, V.data_ptr(), V.stride(0)
        V = np.asarray(V)
        if V.ndim != 2 or V.shape[0] != self.nrows():
            raise HifAmdError(2, f"{name}: expected an [nrows][c] block")
        if np.iscomplexobj(V) and self.dtype.kind != "c":
            raise HifAmdError(2, f"{name}: a complex block on a {self.dtype} hierarchy")
        V = np.ascontiguousarray(V, dtype=self.dtype)
        return V, _p(V), V.shape[1]

    def b_project(self, W, Y, gen=False):
        """The B-orthogonal projector W <- W - Y (B Y)^H W in place (hifamd_eig_project / _dev): Y [n][m], m <= 128, with
        B-orthonormal columns (not checked), W [n][kw], kw <= 16; B = I, or with gen the mass matrix of set_mass_matrix.
        W: a C-contiguous host array of the handle's dtype, or a CUDA tensor with unit column stride (any row stride); Y
        the same kind.  Returns W."""
        dev = _is_torch(W)
        Y, py, ldy = self._eig_block(Y, "Y", dev)
        if dev:
            W2 = self._dev_block(W, "W")
            if W2.data_ptr() != W.data_ptr():
                raise HifAmdError(2, "W: blocks must be row-interleaved (unit column stride)")
            _check(lib().hifamd_eig_project_dev(self._h, int(bool(gen)), Y.shape[1], py, ldy, W2.shape[1], W2.data_ptr(),
                                                W2.stride(0)))
            return W
        if not isinstance(W, np.ndarray) or W.dtype != self.dtype or not W.flags.c_contiguous or W.ndim != 2 \
                or W.shape[0] != self.nrows():
            raise HifAmdError(2, f"W: expected a C-contiguous {self.dtype} array of shape (n, kw)")
        _check(lib().hifamd_eig_project(self._h, int(bool(gen)), Y.shape[1], py, ldy, W.shape[1], _p(W), W.shape[1]))
        return W

    def eigsh(self, nev, k=16, guard=None, gen=False, Y=None, X0=None, seed=0, tol=1e-8, maxit=200, deftol=1e-12,
              full_rank=False):
        """The nev smallest eigenpairs of the matrix of set_matrix (gen: of the pencil with the mass matrix of
        set_mass_matrix) by locked LOBPCG sweeps (hifamd_eigs / _dev): blocks of k <= 16 candidates with `guard` guard
        columns (default max(1, k // 4); 0 for k = 1), every sweep locks its leading converged columns into a block of
        B-orthonormal constraints that all later search directions are projected against.  Y ([n][m0], B-orthonormal,
        m0 + nev <= 128): constraints to start from -- eigenvectors of an earlier call, or a known null space, which is how
        a singular pencil is deflated.  X0 ([n][k]) or the generated block of `seed` starts the first sweep; maxit is per
        sweep.  Host arrays or CUDA tensors (Y and X0 of one kind).  Returns (lam, X, res, flags, info): lam [nev] in lock
        order, X [n][nev] with X^H B X = I and Y^H B X = 0, res [nev], flags [nev] 0 locked / 1 breakdown / 2 not
        converged, info = (total steps, sweeps, locked, smallest basis rank); last_eigsh_sweeps keeps the sweeps'
        (want, locked, steps)."""
        k = int(k) if X0 is None else int(X0.shape[1])
        if guard is None:
            guard = max(1, k // 4) if k > 1 else 0
        given = [v for v in (Y, X0) if v is not None]
        dev = bool(given) and _is_torch(given[0])
        py, ldy, m0 = None, 0, 0
        if Y is not None:
            Y, py, ldy = self._eig_block(Y, "Y", dev)
            m0 = int(Y.shape[1])
        px0, ldx0 = None, 0
        if X0 is not None:
            X0, px0, ldx0 = self._eig_block(X0, "X0", dev)
        nev = int(nev)
        cols = max(nev, 1)
        if dev:
            import torch

            X = torch.empty((self.nrows(), cols), dtype=given[0].dtype, device=given[0].device)
            px, ldx = X.data_ptr(), X.stride(0)
        else:
            X = np.empty((self.nrows(), cols), dtype=self.dtype)
            px, ldx = _p(X), cols
        lam, res = np.zeros(cols), np.zeros(cols)
        fl, info = np.zeros(cols, dtype=np.int32), np.zeros(4, dtype=np.int32)
        fn = lib().hifamd_eigs_dev if dev else lib().hifamd_eigs
        _check(fn(self._h, int(bool(gen)), nev, k, int(guard), py, ldy, m0, px0, ldx0, int(seed), float(tol), float(deftol),
                  int(maxit), -1 if full_rank else 0, _p(lam), px, ldx, _p(res), _p(fl), _p(info)))
        sweeps = np.zeros((max(int(info[1]), 1), 3), dtype=np.int32)
        ns = lib().hifamd_eigs_sweeps(self._h, _p(sweeps), sweeps.shape[0])
        self.last_eigsh_sweeps = [tuple(int(v) for v in row) for row in sweeps[:max(ns, 0)]]
        return lam, X, res, fl, info

    def bgcr(self, b, block=64, restart=10, rtol=1e-6, maxit=500, deftol=1e-12, full_rank=False):
        """Restarted block GCR (x0 = 0; block GMRES(restart) with right preconditioning in exact arithmetic) for a general
        pair (A, M) (hifamd_bgcr_batch / _dev): the columns of b ([n] or [n][nrhs], host array or CUDA tensor) are cut into
        tiles of `block` <= 64, and the columns of a tile share one block Krylov space, as in bcg -- but nothing is asked of
        the hierarchy.  The residual is kept factored and rank-revealed (a pivoted Cholesky that drops pivots <= deftol), and
        every flag 0 is decided on a true residual b - A x at the start of a cycle of at most `restart` <= 64 steps.  Needs
        set_matrix.  Returns (x, flags, iters, ranks); ints for a vector, ranks always an array: per tile its rank after the
        start of its first cycle and during its last step.  flags: 0 converged, 1 stagnated, a bad Gram or a non-finite
        column, 2 reached maxit; iters: the steps (one apply plus one SpMM each) of the column's tile.  A column's result
        depends on the columns it shares a tile with."""
        ntile = -(-(1 if b.ndim == 1 else int(b.shape[1])) // max(int(block), 1))
        ranks = np.zeros(2 * max(ntile, 1), dtype=np.int32)
        x, fl, it = self._krylov("bgcr", b, int(block), int(restart), rtol=rtol, maxit=maxit, full_rank=full_rank,
                                 mid=(float(deftol),), tail=(_p(ranks),))
        return x, fl, it, ranks

    def sqmr(self, b, rtol=1e-6, maxit=500, full_rank=False):
        """Symmetric QMR (Freund / Nachtigal, x0 = 0) for a Hermitian pair (A, M) that may be indefinite, all columns of b
        ([n] or [n][nrhs], host array or CUDA tensor) in lock step on the device.  Needs set_matrix and is_hermitian().
        One apply plus one SpMM per iteration.  Returns (x, flags, iters); ints for a vector.  flags: 0 converged,
        1 breakdown, 2 reached maxit."""
        return self._krylov("sqmr", b, rtol=rtol, maxit=maxit, full_rank=full_rank)

    def bicgstab(self, b, rtol=1e-6, maxit=500, full_rank=False):
        """Right-preconditioned BiCGSTAB (x0 = 0, shadow residual b) for a general pair (A, M), all columns of b ([n] or
        [n][nrhs], host array or CUDA tensor) in lock step on the device.  Needs set_matrix.  maxit and iters count
        steps (one apply plus one SpMM each; two per iteration).  Returns (x, flags, iters); ints for a vector.
        flags: 0 converged, 1 breakdown, 2 reached maxit."""
        return self._krylov("bicgstab", b, rtol=rtol, maxit=maxit, full_rank=full_rank)

    def idrs(self, b, s=4, rtol=1e-6, maxit=500, full_rank=False, P=None, seed=0):
        """Right-preconditioned IDR(s) with biorthogonalization (x0 = 0) for a general pair (A, M), all columns of b ([n] or
        [n][nrhs], host array or CUDA tensor) in lock step on the device (hifamd_idrs_batch / _dev).  Needs set_matrix.
        s: 1 .. 8.  P: the [n][s] shadow block (a host array, used as given, one block for all columns), or None: generated
        on the device from seed.  maxit and iters count steps (one apply plus one SpMM each; s + 1 per cycle).  Returns
        (x, flags, iters); ints for a vector.  flags: 0 converged, 1 breakdown, 2 reached maxit."""
        if P is None:
            lead = (int(s), None, 0, int(seed))
        else:
            P = np.ascontiguousarray(P, dtype=self.dtype)
            if P.ndim != 2 or P.shape[0] != self.nrows():
                raise HifAmdError(2, "idrs: P must be [n][s]")
            lead = (int(s), _p(P), P.shape[1], int(seed))
        return self._krylov("idrs", b, *lead, rtol=rtol, maxit=maxit, full_rank=full_rank)

    def fgmres(self, b, restart=30, rtol=1e-6, maxit=500, full_rank=False):
        """Flexible GMRES with 2^k refinement sweeps as the preconditioner of outer cycle k (the reference's
        fgmres_hifir, examples/advanced/gmres.hpp:127-231); host arrays.  Returns (x, flags, iters, sweeps)."""
        vec = (b.ndim == 1)
        B = np.ascontiguousarray(b, dtype=self.dtype).reshape(b.shape[0], -1)
        X = np.empty_like(B)
        fl, it, mv = (np.zeros(B.shape[1], dtype=np.int32) for _ in range(3))
        _check(lib().hifamd_fgmres_batch(self._h, _p(B), B.shape[1], _p(X), X.shape[1], B.shape[1], int(restart),
                                        float(rtol), int(maxit), -1 if full_rank else 0, _p(fl), _p(it), _p(mv)))
        if vec:
            return X.reshape(-1), int(fl[0]), int(it[0]), int(mv[0])
        return X, fl, it, mv

    def time_apply(self, B, X, rank=0, warmup=2, reps=10):
        """Average device milliseconds of one batched apply, HIP events on the handle's stream."""
        self._dev_block(B, "B")
        self._dev_block(X, "X", B.shape)
        ms = C.c_double()
        _check(lib().hifamd_time_apply(self._h, B.data_ptr(), B.stride(0), X.data_ptr(), X.stride(0), B.shape[1],
                                      int(rank), int(warmup), int(reps), C.byref(ms)))
        return ms.value

    def sync(self):
        _check(lib().hifamd_sync(self._h))
