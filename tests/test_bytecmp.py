"""rf_bytecmp.hpp: the byte compares of the hamming / prefix / postfix kernels (rf_compare.hip) are `__host__ __device__` inlines;
tests/cpp/bytecmp_check.cpp compiles the same header with the host compiler and holds it to byte loops -- all 256 x 256 byte pairs in each lane of a
dword, the tail lengths 0..16, every [from, to) mask of a chunk, whole chunks that hold the symbol 0, and the realigned query read.  Once plainly,
once under the host sanitizers."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bytecmp_check.cpp")
INC = os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_byte_helpers_match_the_byte_loops(tmp_path, flags):
    exe = tmp_path / "bytecmp_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", INC, "-o", str(exe), SRC], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"checks (\d+) mismatches 0\b", r.stdout)
    assert m and int(m.group(1)) > 4 * 256 * 256 * 4, r.stdout


def test_the_kernels_compile_the_checked_header():
    src = open(os.path.join(INC, "rf_compare.hip")).read()
    assert '#include "rf_bytecmp.hpp"' in src
    for name in ("chunk_nonzero_bytes", "chunk_first_nonzero", "chunk_last_nonzero", "keep_range", "differ_outside", "align_bytes"):
        assert name + "(" in src, name
