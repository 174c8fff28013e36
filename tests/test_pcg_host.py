"""CPU: the Hermitian test behind hifamd_pcg_batch (hifamd_hermitian / HIF.is_hermitian) on the golden fixtures and on
copies with a single defect each, before hifamd_finalize and without a GPU; and no CPU fallback for pcg."""
import copy

import numpy as np
import pytest

import hifir_amd
from hifir_amd._lib import lib
from util import load_hier


def _import(levels, dense=True, dtype=None):
    """add_level / set_dense* as HIF.from_levels does, without finalize (no GPU needed)."""
    if dtype is None:
        dtype = np.complex128 if any(np.iscomplexobj(lv["L_vals"]) or np.iscomplexobj(lv["d"]) or
                                     np.iscomplexobj(lv["E_vals"]) for lv in levels) else np.float64
    M = hifir_amd.HIF(dtype)
    for lv in levels:
        M.add_level(lv)
    last = levels[-1]
    if dense and int(last.get("dense_n", 0)) > 0:
        if int(last.get("dense_lup", 0)):
            M.set_dense_lup(last["dense"])
        elif int(last.get("dense_symm", 0)):
            M.set_dense_symm(last["dense"], int(last.get("spd", 0)))
        else:
            M.set_dense(last["dense"])
    return M


def _verdict(M):
    """(hifamd_hermitian, message of the first violation or None)"""
    h = lib().hifamd_hermitian(M._h)
    msg = lib().hifamd_last_error()
    return h, (msg.decode() if (h == 0 and msg) else None)


def _mirror(lv, fix_lu=True, fix_ef=True):
    """U_B := L_B^H and / or F := E^H of one level (CCS arrays rebuilt with scipy)."""
    import scipy.sparse as sp

    m, n = int(lv["m"]), int(lv["n"])
    out = dict(lv)

    def put(name, A):
        A = sp.csc_matrix(A)
        A.sort_indices()
        out[name + "_colptr"] = A.indptr.astype(np.int64)
        out[name + "_rowind"] = A.indices.astype(np.int32)
        out[name + "_vals"] = A.data.copy()

    if fix_lu:
        L = sp.csc_matrix((lv["L_vals"], lv["L_rowind"], lv["L_colptr"]), shape=(m, m))
        put("U", L.conj().T)
    if fix_ef and n > m:
        E = sp.csc_matrix((lv["E_vals"], lv["E_rowind"], lv["E_colptr"]), shape=(n - m, m))
        put("F", E.conj().T)
    return out


def test_null_handle():
    assert lib().hifamd_hermitian(None) == -1


def test_symmetric_factorization_is_hermitian():
    levels, _ = load_hier("p2d_32_symm")
    M = _import(levels)
    assert M.is_hermitian()
    assert _verdict(M) == (1, None)


@pytest.mark.parametrize("name,level,what", [
    ("p2d_30", 1, "QRCP"),            # sparse level mirrored bit for bit: only the dense last level fails
    ("p2d_30_lup", 1, "LUP"),
    ("cd2d_48", 0, "U_B != L_B^H"),   # nonsymmetric matrix
    ("p2d_100_tuned", 1, "U_B != L_B^H"),  # nonsymmetric factorization of a symmetric matrix: off by 1.7e-16 at level 1
    ("herm_24_symm", 0, "F != E^H"),  # complex is_symm fixture: E == F^T, not F^H
])
def test_fixtures_that_are_not_hermitian(name, level, what):
    levels, _ = load_hier(name)
    M = _import(levels)
    assert not M.is_hermitian()
    h, msg = _verdict(M)
    assert h == 0
    assert msg.startswith(f"level {level}: ") and what in msg, msg


def test_each_fixture_fails_for_its_own_reason():
    # p2d_30 / p2d_30_lup: the same sparse level passes without the last level, and with a SYEIG block instead
    for name in ("p2d_30", "p2d_30_lup"):
        levels, _ = load_hier(name)
        assert _import(levels, dense=False).is_hermitian()
        sym = copy.deepcopy(levels)
        sym[-1]["dense_lup"] = 0
        sym[-1]["dense_symm"] = 1
        assert _import(sym).is_hermitian()
    # cd2d_48: L != U^T, and F != E^T behind it; mirrored, only its QRCP block remains
    levels, _ = load_hier("cd2d_48")
    h, msg = _verdict(_import([_mirror(levels[0], fix_ef=False)] + levels[1:]))
    assert msg == "level 0: F != E^H"
    h, msg = _verdict(_import([_mirror(lv) for lv in levels]))
    assert msg.startswith("level 2: ") and "QRCP" in msg
    # p2d_100_tuned: level 1 by one rounding, level 2 by 0.04 and s != t
    levels, _ = load_hier("p2d_100_tuned")
    h, msg = _verdict(_import([levels[0], _mirror(levels[1]), levels[2]]))
    assert msg == "level 2: U_B != L_B^H"
    h, msg = _verdict(_import([levels[0], _mirror(levels[1]), _mirror(levels[2])]))
    assert msg == "level 2: s != t"
    # herm_24_symm: L_B == U_B^H, but F == E^T and d is complex
    levels, _ = load_hier("herm_24_symm")
    h, msg = _verdict(_import([_mirror(levels[0], fix_lu=False)]))
    assert msg == "level 0: Im d != 0"
    assert np.abs(np.imag(levels[0]["d"])).max() > 0.04


def _p2d_32_copy():
    levels, _ = load_hier("p2d_32_symm")
    return copy.deepcopy(levels)


def test_single_defects_are_refused():
    # one U value off by one ulp
    lv = _p2d_32_copy()
    lv[0]["U_vals"] = lv[0]["U_vals"].copy()
    lv[0]["U_vals"][7] = np.nextafter(lv[0]["U_vals"][7], np.inf)
    assert _verdict(_import(lv)) == (0, "level 0: U_B != L_B^H")
    # one t entry changed
    lv = _p2d_32_copy()
    lv[1]["t"] = lv[1]["t"].copy()
    lv[1]["t"][3] *= 2.0
    assert _verdict(_import(lv)) == (0, "level 1: s != t")
    # two entries of q swapped (q_inv kept its inverse, as the import requires)
    lv = _p2d_32_copy()
    q = lv[0]["q"].copy()
    q[[0, 1]] = q[[1, 0]]
    lv[0]["q"] = q
    lv[0]["q_inv"] = np.argsort(q).astype(np.int32)
    assert _verdict(_import(lv)) == (0, "level 0: p != q")
    # complex copy: Hermitian as it stands, refused with Im d != 0
    lv = _p2d_32_copy()
    for L in lv:
        for k in ("L_vals", "U_vals", "E_vals", "F_vals", "d", "dense"):
            if k in L:
                L[k] = np.asarray(L[k]).astype(np.complex128)
    assert _import(lv).is_hermitian()
    lv[1]["d"][5] += 1e-3j
    assert _verdict(_import(lv)) == (0, "level 1: Im d != 0")


def test_the_verdict_follows_the_import():
    # computed once, but a later import call (here: the dense block) is taken into account
    levels, _ = load_hier("p2d_30")
    M = _import(levels, dense=False)
    assert M.is_hermitian()
    M.set_dense(levels[-1]["dense"])
    assert not M.is_hermitian()


def test_pcg_has_no_cpu_fallback():
    levels, d = load_hier("p2d_32_symm")
    M = _import(levels)
    with pytest.raises(hifir_amd.HifAmdError) as e:
        M.pcg(d["b"])  # not finalized: never a CPU result
    assert e.value.code == 3
    if lib().hifamd_device_count() == 0:
        with pytest.raises(hifir_amd.HifAmdError) as e:
            M.finalize(1)
        assert e.value.code == 4 and "no CPU fallback" in e.value.msg
        with pytest.raises(hifir_amd.HifAmdError):
            M.pcg(d["b"])
