"""CPU: the dynamic-LDS layouts of the component-band kernels (hifir_amd/csrc/band_lds.hpp) as a plain C++ program.  The
header is the one statement of each layout: the kernels take their LDS pointers from it, the engine and the k_band_ls planner
their byte counts.  tests/cpp/band_lds_test.cpp walks the sizes the engine can pass and asserts order, no overlap, alignment
and that the last array ends inside bytes(); bytes() at the default sizes is pinned to the sizes the launches have always
asked for.  No GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_lds_layout_program(tmp_path):
    exe = str(tmp_path / "band_lds_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-fsanitize=undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "band_lds_test.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode()
    print(out)
    assert out.strip().endswith("OK") and "FAILED" not in out and "failures 0" in out, out
    # (the sparse layouts alone: 64 own-entry caps x (3 layouts x 240 row counts + 255 black-row counts))
    assert int(re.search(r"argument sets (\d+)", out).group(1)) >= 64 * (3 * 240 + 255)

