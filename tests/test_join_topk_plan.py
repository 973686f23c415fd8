"""The span rule of rf_join_topk_u32 (rapidfuzz_rs_amd/csrc/rf_join_plan.hpp join_topk_span / join_topk_seg_units) holds no HIP call, so the host compiler can
include it: tests/cpp/join_topk_plan_check.cpp builds, for random batches over random corpora, the work lists under the span the rule gives -- for an automatic
target and for the forced targets 1 and 2^20 -- and checks that every (query, tile of its window) lies in exactly one unit, that every unit's ordinal within its
item is below the segment's unit capacity, and that join_valid() accepts the lists.  Once plainly, once under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]}


@pytest.mark.parametrize("build", list(FLAGS))
def test_every_tile_lies_in_one_unit_and_every_unit_in_its_segment(tmp_path, build):
    exe = str(tmp_path / f"join_topk_plan_check_{build}")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *FLAGS[build], "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "join_topk_plan_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    m = re.search(r"join topk plan: (\d+) lists, (\d+) units, (\d+) \(query, tile\) pairs, failures 0", out)
    assert m, out[-3000:]
    assert int(m.group(1)) > 1000 and int(m.group(2)) > 10000 and int(m.group(3)) > 100000


def test_the_kernel_and_the_host_compile_the_checked_header():
    kernel = open(os.path.join(CSRC, "rf_join_topk.hip")).read()
    host = open(os.path.join(CSRC, "rf_api_join.hip")).read()
    assert '#include "rf_join_plan.hpp"' in kernel and '#include "rf_join_plan.hpp"' in host
    assert "join_unit(" in kernel and "join_valid(" in kernel  # the kernel walks the checked lookup, its launcher runs the checked validation
    assert "join_topk_span(" in host and "join_topk_seg_units(" in host
    plan = open(os.path.join(CSRC, "rf_join_plan.hpp")).read()
    assert "hip/hip_runtime.h" not in plan
