"""GPU (-m gpu): a C++ user's program (tests/cpp/facade_xp_test.cpp) that reaches the extra-precise residual through the
header-only facade include/hifir_amd.hpp -- set_residual_precision, residual, hifir under the mode, gmres_ir -- on a stand-in
hierarchy with M = A.  It needs no reference headers, so it is compiled here against the library in the tree and run."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_facade_reaches_the_compensated_residual_and_gmres_ir(tmp_path):
    exe = str(tmp_path / "facade_xp_test")
    libdir = os.path.join(ROOT, "hifir_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_xp_test.cpp"), "-L", libdir, "-lhifir_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "FACADE XP TEST OK" in out.stdout
    assert out.stdout.count(" ok") >= 10 and "FAIL" not in out.stdout
