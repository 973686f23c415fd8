"""rf_dl_cell.hpp: the per-cell update and the packed cell of the Damerau-Levenshtein kernels (rf_damerau.hip) are `__host__ __device__`
inlines; tests/cpp/dl_cell_check.cpp compiles the same header with the host compiler and runs it column by column against a full-matrix
implementation -- the field-width edges (max(len1, len2) = 253, 254, 255, 300) and the query lengths 0, 1, 16, 17, 64, 65 included.  Once
plainly, once under the host sanitizers."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dl_cell_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_dl_cell_matches_the_full_matrix(tmp_path, flags):
    exe = tmp_path / "dl_cell_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-o", str(exe), SRC], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches 0" in r.stdout


def test_the_kernels_compile_the_checked_header():
    src = open(os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc", "rf_damerau.hip")).read()
    assert '#include "rf_dl_cell.hpp"' in src and "dl_step<" in src
