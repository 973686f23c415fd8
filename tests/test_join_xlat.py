"""The row map of the join calls' device road (rapidfuzz_rs_amd/csrc/rf_join_xlat.hpp) holds no HIP call, so the host compiler can include it:
tests/cpp/join_xlat_check.cpp builds it for random pairs of corpora -- bytes or `char` on either side, more than 254 symbols on either side, symbols above the BMP,
symbols of one corpus inside the other's overflow set, symbols the other corpus never stores -- and checks row_of and bad against the definition applied symbol
by symbol (resolve()'s rule), any_bad, the absent row, and the byte x byte identity row_of[s] == sigma_c[inv_sigma_q[s]].  Once plainly, once under
AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]}


@pytest.mark.parametrize("build", list(FLAGS))
def test_row_map_follows_the_definition_symbol_by_symbol(tmp_path, build):
    exe = str(tmp_path / f"join_xlat_check_{build}")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *FLAGS[build], "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "join_xlat_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    m = re.search(r"join xlat: (\d+) pairs, (\d+) symbols, (\d+) bad values, (\d+) absent, (\d+) in the other's overflow, (\d+) above the BMP, (\d+) with over 254 symbols, "
                  r"(\d+) byte identities, failures 0", out)
    assert m, out[-3000:]
    pairs, symbols, bad, absent, overflow, above_bmp, big, identities = (int(g) for g in m.groups())
    # every kind of case the map has to get right was met, many times over
    assert pairs == 3000 and symbols > 100000
    assert bad > 1000 and absent > 1000 and overflow > 1000 and above_bmp > 1000 and big > 500 and identities == 750


def test_the_kernel_and_the_host_compile_the_checked_header():
    kernel = open(os.path.join(CSRC, "rf_join.hip")).read()
    assert "row_of" in kernel and "inv_sigma" not in kernel
    host = open(os.path.join(CSRC, "rf_api_join.hip")).read()
    assert '#include "rf_join_xlat.hpp"' in host and "join_xlat_build(" in host
    header = open(os.path.join(CSRC, "rf_join_xlat.hpp")).read()
    assert "hip_runtime" not in header and "__global__" not in header and '#include "rf_host.hpp"' not in header
