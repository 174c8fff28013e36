"""CPU: the streamed-source plan of sparse-own L bands (host.hpp ls_reorder_own / build_ls_plan / check_ls_plan, kernel
k_band_ls) as a plain C++ program under ASan / UBSan: tests/cpp/ls_plan_test.cpp emulates the kernel's phases from the plan
arrays and compares them bitwise with the row-by-row substitution over the reordered lists, on synthetic triangles and on
the golden hierarchies whose level 0 plans sparse-own components.  No GPU needed."""
import os
import re
import subprocess

import numpy as np

import hifir_amd
from util import HIER_NAMES, load_hier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _save(name, tmp_path):
    levels, d = load_hier(name)
    if np.iscomplexobj(d["b"]):
        return None
    M = hifir_amd.HIF(dtype=d["b"].dtype)
    for lv in levels:
        M.add_level(lv)
    if int(levels[-1].get("dense_n", 0)) > 0:
        M.set_dense(levels[-1]["dense"])
    path = str(tmp_path / f"{name}.hifamd")
    M.save(path)
    return path


def test_streamed_source_plan_program(tmp_path):
    exe = str(tmp_path / "ls_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ls_plan_test.cpp"), "-o", exe])
    files = [p for p in (_save(name, tmp_path) for name in HIER_NAMES) if p]
    assert len(files) >= 8
    env = dict(os.environ, HIFIR_AMD_CD_SPARSE_MIN_ROWS="0")  # sparse-own components on every shallow thin triangle
    for k in ("HIFIR_AMD_DENSE_BLOCK", "HIFIR_AMD_CD_SPARSE_ROWS", "HIFIR_AMD_CD_ROWS"):
        env.pop(k, None)
    out = subprocess.check_output([exe] + files, env=env).decode()
    assert out.strip().endswith("OK"), out
    assert "FAILED" not in out and "failures 0" in out, out
    # the synthetic triangles reach components of several chunks; the golden hierarchies contribute qualifying bands
    assert re.search(r"\((\d+) with more than one chunk\)", out) and int(re.search(r"\((\d+) with more than one chunk\)", out).group(1)) > 0
    per_file = {os.path.basename(m.group(1)): int(m.group(2)) for m in re.finditer(r"^(\S+\.hifamd): (\d+) qualifying L bands$", out, re.M)}
    assert len(per_file) == len(files), out
    assert per_file["p2d_64_deep.hifamd"] > 0 and per_file["p2d_100_tuned.hifamd"] > 0, per_file  # (level 0: components of their own)
    assert "bitwise differences 0" in out and not re.search(r"bitwise differences [1-9]", out), out
