"""CPU: the engine's creation-time options (hifir_amd/csrc/options.hpp) as a plain C++ program.  The header is the one
statement of every switch's name, default and normalisation; tests/cpp/options_test.cpp holds, as literals, what the engine's
constructor computed when it read the environment line by line, and asserts that EngineOptions::from_env gives the same for
real and for complex handles: with nothing set, with every row of the table set alone, at the edges of the derived rules, and
that the table names no variable twice and misses none.  No GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_program(tmp_path):
    exe = str(tmp_path / "options_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-fsanitize=undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "hifir_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "options_test.cpp"), "-o", exe])
    # (the program clears every HIFIR_AMD_* variable itself; one is set here to show that it does)
    out = subprocess.check_output([exe], env=dict(os.environ, HIFIR_AMD_CD_ROWS="64")).decode()
    print(out)
    assert out.strip().endswith("OK") and "FAILED" not in out and "failures 0" in out, out
    assert int(re.search(r"rows (\d+)", out).group(1)) == 56
