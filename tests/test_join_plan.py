"""The work list of rf_join_u32 (rapidfuzz_rs_amd/csrc/rf_join_plan.hpp) holds no HIP call, so the host compiler can include it: tests/cpp/join_plan_check.cpp
builds, for random multisets of query lengths, corpora and cutoffs, the items and the prefix table batch by batch and checks that every (query, tile in its window)
is covered by exactly one work item, that no item mixes the classes, that the prefix table maps every workgroup unit -- through join_unit(), the function the kernel
runs -- into a valid (item, sub-range) and covers every sub-range once, and that join_valid() refuses lists that name a tile beyond the corpus or a table beyond the
batch.  Once plainly, once under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]}


@pytest.mark.parametrize("build", list(FLAGS))
def test_work_list_covers_every_query_tile_once(tmp_path, build):
    exe = str(tmp_path / f"join_plan_check_{build}")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *FLAGS[build], "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "join_plan_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    m = re.search(r"join plan: (\d+) lists, (\d+) units, (\d+) \(query, tile\) pairs, failures 0", out)
    assert m, out[-3000:]
    assert int(m.group(1)) > 1000 and int(m.group(2)) > 10000 and int(m.group(3)) > 100000


def test_the_kernel_and_the_host_compile_the_checked_header():
    kernel = open(os.path.join(CSRC, "rf_join.hip")).read()
    assert '#include "rf_join_plan.hpp"' in kernel and "join_unit(" in kernel and "join_valid(" in kernel
    host = open(os.path.join(CSRC, "rf_api_join.hip")).read()
    assert '#include "rf_join_plan.hpp"' in host and "join_items(" in host and "join_sort(" in host
    header = open(os.path.join(CSRC, "rf_join_plan.hpp")).read()
    assert "hip_runtime" not in header and "__global__" not in header
