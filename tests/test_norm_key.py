"""rf_norm_key.hpp: the 32-bit score image of rf_topk_multi_f64's in-scan lists and its inverse are `__host__ __device__` inlines;
tests/cpp/norm_key_check.cpp compiles the same header with the host compiler and checks the f64-seeded key against its integer definition, the
key's order against the order of the doubles, equal keys <=> equal doubles, and norm_key_ratio as the inverse whose quotient has the bits of
dist / maximum -- exhaustively for maximum <= 1024, on 12 000 Farey-neighbour pairs with denominators in 60000 .. 65535, and on the edges
(dist == maximum, maximum == 0, maximum == 65535).  Once plainly, once under the host sanitizers."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "norm_key_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_norm_key_matches_its_definition_and_inverts(tmp_path, flags):
    exe = tmp_path / "norm_key_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-o", str(exe), SRC], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches 0" in r.stdout
    assert "farey neighbour pairs: 12000" in r.stdout


def test_the_kernel_and_the_host_compile_the_checked_header():
    csrc = os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc")
    kernel = open(os.path.join(csrc, "rf_topk_multi.hip")).read()
    assert '#include "rf_norm_key.hpp"' in kernel and "norm_key_scaled(" in kernel
    host = open(os.path.join(csrc, "rf_api_topk_multi.hip")).read()
    assert '#include "rf_norm_key.hpp"' in host and "norm_key_ratio(" in host
