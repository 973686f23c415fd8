"""The host half of rf_filter_multi_f64 -- ordering a fused member's key row and turning the keys back into (index, double) pairs,
rapidfuzz_rs_amd/csrc/rf_filter_multi_rows.hpp -- includes nothing of HIP: tests/cpp/filter_multi_f64_rows_check.cpp compiles it with the host
compiler under the host sanitizers and compares every pair with a direct (double)dist / (double)maximum computation: equal ratios from different
(dist, maximum) pairs tied by index, key 0, the clamp 0xFFFFFFFF, both ops, the three orders."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "filter_multi_f64_rows_check.cpp")


def test_rows_decode_and_order_under_the_host_sanitizers(tmp_path):
    exe = tmp_path / "filter_multi_f64_rows_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rows ok" in r.stdout


def test_the_api_calls_the_checked_function_and_the_kernel_the_checked_key():
    api = open(os.path.join(CSRC, "rf_api_filter_multi.hip")).read()
    assert '#include "rf_filter_multi_rows.hpp"' in api and "filter_multi_f64_row(" in api
    rows = open(os.path.join(CSRC, "rf_filter_multi_rows.hpp")).read()
    assert "#include <hip" not in rows and "norm_key_ratio(" in rows
    kernel = open(os.path.join(CSRC, "rf_filter_multi.hip")).read()
    assert '#include "rf_norm_key.hpp"' in kernel and "norm_key_scaled(" in kernel
